"""The device beam search's definition, checked without a device: tests/beam_ref.py (the numpy restatement of
include/bqhip_beam.h that the GPU tests hold the kernels to) decides what generation.beam_search decides on every case of
tests/beam_cases.py, every case keeps its decision margins, the header is additive and bound from its own text, and
generate(device_beams=True) leaves every ineligible decode on today's path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import beam_cases as C
import beam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.decode_cases()


@pytest.fixture(scope="module")
def runs():
    return {C.case_id(p): C.run_case(p) for p in CASES}


def torch_oracle(orc, nb):
    A, Ct = torch.from_numpy(orc["A"]), torch.from_numpy(orc["C"])

    def step_fn(ids, past):
        return A[ids.shape[1] - 1, torch.arange(ids.shape[0]) // nb] + Ct[ids[:, -1] % 64], None
    return step_fn


@pytest.mark.parametrize("p", CASES, ids=C.case_id)
def test_reference_decides_what_beam_search_decides(p, runs):
    from bridgeqa_amd.generation import beam_search
    r = runs[C.case_id(p)]
    ids = torch.full((p["B"] * p["nb"], 1), C.BOS, dtype=torch.long)
    seq, scores = beam_search(torch_oracle(R.make_oracle(p), p["nb"]), lambda past, idx: past, ids, p["nb"], p["max_length"],
                              p["eos"], p["pad"], min_length=p["min_length"], length_penalty=p["length_penalty"],
                              early_stopping=p["early_stopping"])
    assert seq.numpy().tolist() == r["seq"].tolist()
    assert float(np.abs(scores.numpy().astype(np.float64) - r["scores"]).max()) <= 1e-6


@pytest.mark.parametrize("extra", [1, None])
def test_steps_after_all_done_change_nothing(extra, runs):
    early = [p for p in CASES if runs[C.case_id(p)]["all_done"]]
    assert early
    for p in early:
        r, more = runs[C.case_id(p)], C.run_case(p, extra_steps=extra)
        assert more["steps"] > r["steps"]
        assert more["seq"].tolist() == r["seq"].tolist() and more["scores"].tolist() == r["scores"].tolist()


def test_every_case_keeps_its_margins(runs):
    worst = min((r["min_margin"], k) for k, r in runs.items())
    print("smallest decision margin over %d cases: %.3e (%s)" % (len(runs), worst[0], worst[1]))
    low = [(k, r["min_margin"]) for k, r in runs.items() if not r["min_margin"] >= C.MARGIN]
    assert not low, low


def test_the_cases_cover_what_they_must(runs):
    assert {p["nb"] for p in CASES} >= {1, 2, 5, 10, 16}
    for nb in (1, 2, 5, 10, 16):
        assert {p["V"] for p in CASES if p["nb"] == nb} >= {2 * nb + 1, 50, 200}
    assert {p["min_length"] for p in CASES} >= {0, 1, 3} and {p["length_penalty"] for p in CASES} >= {1.0, 0.0, 2.0}
    assert {p["early_stopping"] for p in CASES} == {False, True}
    for what in ("all_done", "mixed", "evicted", "ignored_eos"):
        n = sum(bool(r[what]) for r in runs.values())
        print("%s: %d cases" % (what, n))
        assert n >= 1, what


def test_the_order_is_total_and_breaks_ties_by_index():
    s = np.array([1.0, np.nan, 1.0, -0.0, 0.0, np.inf, -np.inf, np.nan], np.float32)
    assert R.ranked(s, 8).tolist() == [1, 7, 5, 0, 2, 3, 4, 6]
    big = np.zeros(1000, np.float32)
    big[[7, 400, 999]] = 2.0
    assert R.ranked(big, 6).tolist() == [7, 400, 999, 0, 1, 2]
    # -1e9 + x rounds to -1e9 for |x| < 32: the closed beams of step 0 collide, the index decides
    assert np.float32(-1e9) + np.float32(-31.0) == np.float32(-1e9)


def test_emulated_summation_order_stays_inside_the_bound():
    """K was fixed from this emulation (beam_cases.EMU_WORST) before any device run; hold the emulation itself to K"""
    for B, nb, V in ((1, 16, 33), (3, 5, 33), (1, 10, 200)):
        p = C.step_params(B, nb, V, 0)
        st, logits = C.state_at(p, 1)
        emu = R.emu_scores(logits, st["beam_score"], st["cur_len"], p, head=V % 2)
        err, e32, ulp = R.score_errors(emu, logits, st["beam_score"], st["cur_len"], p)
        assert float(err[np.isfinite(err)].max()) <= C.K * e32 + ulp


def test_header_is_c99_additive_and_bound(tmp_path):
    from bridgeqa_amd import _cabi, _ext
    assert "bqhip_beam.h" in _cabi.ADDITIVE_HEADERS
    assert list(_cabi.EXTENSION_PROTOS) == ["bqx_beam_step"]
    assert "bqx_beam_step" not in _cabi.PROTOS and "bqx_beam_step" not in _cabi.ADDITIVE_PROTOS
    restype, argtypes = _cabi.EXTENSION_PROTOS["bqx_beam_step"]
    struct = _cabi.ADDITIVE_STRUCTS["bq_beam_state"]
    assert restype is _cabi.ctypes.c_int and argtypes == [_cabi.ctypes.POINTER(struct), _cabi.ctypes.c_void_p]
    assert _ext._lib.bqx_beam_step.argtypes == argtypes
    # the struct is the header's: field names and order, one tensor per pointer field after `logits`
    text = open(os.path.join(ROOT, "include", "bqhip_beam.h")).read()
    body = text[text.index("typedef struct bq_beam_state {"):text.index("} bq_beam_state;")]
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    fields = [n for n, _ in struct._fields_]
    assert names == fields and fields[:12] == ["B", "nb", "V", "max_length", "Lmax", "eos", "pad", "min_length",
                                               "early_stopping", "logits_bf16", "ld_logits", "logits"]
    assert set(fields[12:]) == set(_ext._BEAM_FIELDS)
    assert _cabi.DEFINES["BQHIP_ABI_VERSION"] == 6 and len(_cabi.PROTOS) == 97
    assert (_ext.BEAM_MAX_NB, _ext.BEAM_MAX_LEN) == (16, 64) and len(_ext.BEAM_CALLS) == 1
    assert '#include "bqhip_beam.h"' in open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    src = tmp_path / "t.c"
    src.write_text('#include "bqhip_beam.h"\nint main(void) { bq_beam_state s; s.nb = BQ_BEAM_MAX_NB; return s.nb == 16 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_entry_point_is_exported_and_compiled_against_its_declaration(tmp_path):
    """what tests/test_cabi_cpu.py holds the bq_ entry points to, for the bqx_ one: the exported bqx_ symbols are the declared
    ones, the definition is a plain `extern "C"` in a source that includes the header, and one that disagrees does not compile"""
    from bridgeqa_amd import _cabi, _ext
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ext.library_path()]).decode()
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("bqx_")}
    assert exported == set(_cabi.EXTENSION_PROTOS)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bridgeqa_amd", "csrc", "beam.hip")).read())
    heads = re.findall(r"^([^\n;{}]*?)\bbqx_beam_step\s*\(", src, flags=re.M)
    assert heads == ['extern "C" int '] and '#include "bq_common.h"' in src
    assert '#include "bqhip_fusion.h"' in open(os.path.join(ROOT, "bridgeqa_amd", "csrc", "bq_common.h")).read()
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return
    for first, conflict in (("const bq_beam_state *st", False), ("bq_beam_state *st, int n", True)):
        t = str(tmp_path / ("entry%d.hip" % conflict))
        open(t, "w").write('#include "bqhip_fusion.h"\nextern "C" int bqx_beam_step(%s, void *stream) { return 0; }\n' % first)
        r = subprocess.run([hipcc, "--cuda-host-only", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), t],
                           capture_output=True, text=True)
        assert (r.returncode != 0 and "conflicting types" in r.stderr) if conflict else r.returncode == 0, r.stderr


def test_the_beam_kernels_keep_their_lds_and_do_not_spill():
    """tests/golden/kernel_resources_beam.json: LDS / scratch of the kernels of csrc/beam.hip from the compiler's resource
    remarks, held as tests/test_kernel_resources_cpu.py holds the older kernels to their fixture; scratch must be 0"""
    import json
    from bridgeqa_amd import build
    build.build()
    res = build.kernel_resources()
    if res is None:
        pytest.skip("objects were not compiled by this checkout's build.py (prebuilt library)")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_beam.json")))
    mine = {k: v for k, v in res.items() if "beam_" in k}
    assert set(mine) == set(gold) and len(gold) == 4
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 == gold[k]["scratch"], k
        assert v.get("lds", 0) <= gold[k]["lds"], (k, v)


def test_the_switch_defaults_to_off():
    code = "from bridgeqa_amd import med; print(int(med._BEAM_DEVICE[0]))"
    env = {k: v for k, v in os.environ.items() if k != "BQ_BEAM_DEVICE"}
    for value, want in ((None, "0"), ("1", "1")):
        e = dict(env, **({"BQ_BEAM_DEVICE": value} if value is not None else {}))
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])


def small_decoder(vocab, dev, max_positions=80, seed=0):
    from bridgeqa_amd import med
    cfg = med.BertConfig(hidden_size=64, num_attention_heads=4, intermediate_size=128, num_hidden_layers=2, vocab_size=vocab,
                         max_position_embeddings=max_positions, encoder_width=64, pad_token_id=C.PAD)
    cfg.add_cross_attention = True
    torch.manual_seed(seed)
    dec = med.BertLMHeadModel(config=cfg).to(dev).eval()
    with torch.no_grad():
        dec.cls.predictions.bias.copy_(torch.randn(vocab, device=dev) * 1.5)
        dec.cls.predictions.decoder.weight.mul_(8.0)
    return dec


# (what makes it ineligible, vocabulary, beams, max_length, prompt)
INELIGIBLE = [("17 beams", 60, 17, 6, [C.BOS]), ("V = 2 nb", 10, 5, 6, [C.BOS]), ("max_length 65", 30, 2, 65, [C.BOS]),
              ("a prompt of two tokens", 30, 4, 6, [C.BOS, 7]), ("nothing but the CPU tensors", 30, 4, 6, [C.BOS])]


def both_routes(dec, dev, nb, max_length, prompt, B=2):
    """generate with device_beams False and True on the same inputs"""
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(B * nb, 5, dec.config.encoder_width, generator=g).to(dev)
    em = torch.ones(B * nb, 5, dtype=torch.long, device=dev)
    ids = torch.tensor([prompt] * B, dtype=torch.long, device=dev)
    kw = dict(max_length=max_length, min_length=1, num_beams=nb, eos_token_id=C.EOS, pad_token_id=C.PAD,
              encoder_hidden_states=enc, encoder_attention_mask=em, return_scores=True)
    return dec.generate(ids, device_beams=False, **kw), dec.generate(ids, device_beams=True, **kw)


@pytest.mark.parametrize("why,vocab,nb,max_length,prompt", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_decodes_take_todays_path_on_the_cpu(why, vocab, nb, max_length, prompt):
    from bridgeqa_amd import _ext, med
    dec = small_decoder(vocab, torch.device("cpu"))
    calls, decodes = _ext.BEAM_CALLS[0], med._DECODE_STATS["beam_decodes"]
    off, on = both_routes(dec, torch.device("cpu"), nb, max_length, prompt)
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    assert _ext.BEAM_CALLS[0] == calls and med._DECODE_STATS["beam_decodes"] == decodes


def test_fp32_compute_dtype_takes_todays_path_on_the_cpu():
    from bridgeqa_amd import _ext, fusion_ops as ops
    prev = ops.set_compute_dtype(torch.float32)
    try:
        calls = _ext.BEAM_CALLS[0]
        off, on = both_routes(small_decoder(30, torch.device("cpu")), torch.device("cpu"), 4, 6, [C.BOS])
        assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1]) and _ext.BEAM_CALLS[0] == calls
    finally:
        ops.set_compute_dtype(prev)
