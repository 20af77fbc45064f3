"""The attention core of MHAtt (csrc/mhatt.hip) without a GPU: the interface exists from the header to the module switch, the fp32
restatement of the kernels (tests/mhatt_ref.py) stays inside the per-element fp64 bounds on every case, planted defects break
them, and with the switch off -- or on, with host tensors or ineligible inputs -- the modules compute bit for bit what they
computed before the switch existed."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import mhatt_ref as R
from bridgeqa_amd import mcan_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bqh_mhatt_fwd", "bqh_mhatt_bwd_ws_floats", "bqh_mhatt_bwd"]
WORST = {}


def _ratio(name, out, ref, tol):
    r, msg = R.excess(out, ref, tol)
    assert msg is None, "%s: %s" % (name, msg)
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


def _breaks(out, ref, tol):
    return R.excess(out, ref, tol)[1] is not None


# ---- the interface exists (fails without the feature) ---------------------------------------------------------------------------
def test_the_interface_exists_from_the_header_to_the_switch():
    from bridgeqa_amd import _cabi, _ext, build
    assert "bqhip_mhatt.h" in _cabi.ADDITIVE_HEADERS and list(_cabi.MHATT_PROTOS) == NAMES
    assert not set(NAMES) & (set(_cabi.PROTOS) | set(_cabi.ADDITIVE_PROTOS) | set(_cabi.EXTENSION_PROTOS) | set(_cabi.MCAN_PROTOS))
    assert _cabi.DEFINES["BQHIP_ABI_VERSION"] == 6 and _cabi.ADDITIVE_DEFINES["BQ_MHATT_MAX_N"] == 1024 == _ext.MHATT_MAX_N
    vp, i = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int
    assert _cabi.MHATT_PROTOS["bqh_mhatt_fwd"] == (i, [vp] * 7 + [i] * 5 + [vp])
    assert _cabi.MHATT_PROTOS["bqh_mhatt_bwd_ws_floats"] == (_cabi.ctypes.c_long, [i] * 5)
    assert _cabi.MHATT_PROTOS["bqh_mhatt_bwd"] == (i, [vp] * 11 + [i] * 5 + [vp])
    for n in NAMES:
        assert getattr(_ext._lib, n).argtypes == _cabi.MHATT_PROTOS[n][1] and getattr(_ext._lib, n).restype == _cabi.MHATT_PROTOS[n][0]
    for n in ("mhatt_ok", "mhatt_fwd", "mhatt_bwd"):
        assert callable(getattr(_ext, n))
    assert len(_ext.MHATT_CALLS) == 2
    assert callable(mcan_module.set_fused_attention) and mcan_module.fused_attention_enabled() in (False, True)
    assert _ext.mhatt_ok(256, 8, 256, 20) and _ext.mhatt_ok(64, 1, 1, 1024) and not _ext.mhatt_ok(384, 8, 4, 4)
    assert not _ext.mhatt_ok(256, 8, 1025, 4) and not _ext.mhatt_ok(256, 8, 4, 0) and not _ext.mhatt_ok(100, 3, 4, 4)
    lib = _ext._lib
    # the workspace: ds, one float per (sample, head, query, key); 0 for an ineligible size
    assert lib.bqh_mhatt_bwd_ws_floats(3, 8, 37, 9, 32) == 3 * 8 * 37 * 9
    assert lib.bqh_mhatt_bwd_ws_floats(64, 8, 1024, 1024, 64) == 64 * 8 * 1024 * 1024           # past 2^31 bytes: a long
    assert lib.bqh_mhatt_bwd_ws_floats(3, 8, 37, 9, 48) == 0 and lib.bqh_mhatt_bwd_ws_floats(3, 8, 37, 1025, 32) == 0
    # ineligible sizes are BQ_EINVAL before any pointer is looked at
    null7, null11 = [None] * 7, [None] * 11
    assert lib.bqh_mhatt_fwd(*null7, 2, 8, 4, 4, 48, None) == -1 and b"d 48" in lib.bq_last_error()
    assert lib.bqh_mhatt_fwd(*null7, 2, 8, 4, 1025, 32, None) == -1 and b"Nk 1025" in lib.bq_last_error()
    assert lib.bqh_mhatt_fwd(*null7, 2, 0, 4, 4, 32, None) == -1 and b"heads 0" in lib.bq_last_error()
    assert lib.bqh_mhatt_bwd(*null11, 2, 8, 4, 4, 48, None) == -1 and b"d 48" in lib.bq_last_error()
    assert lib.bqh_mhatt_bwd(*null11, 2, 8, 4, 1025, 32, None) == -1 and lib.bqh_mhatt_bwd(*null11, 2, 0, 4, 4, 32, None) == -1
    assert lib.bqh_mhatt_fwd(*null7, 8192, 8, 4, 4, 32, None) == -1 and b"65535" in lib.bq_last_error()      # a grid extent
    assert lib.bqh_mhatt_fwd(*null7, 2, 8, 4, 4, 32, None) == -1 and b"null pointer" in lib.bq_last_error()
    assert lib.bqh_mhatt_bwd(*null11, 2, 8, 4, 4, 32, None) == -1 and b"null pointer" in lib.bq_last_error()
    assert lib.bqh_mhatt_fwd(*null7, 0, 8, 4, 4, 32, None) == 0 and lib.bqh_mhatt_bwd(*null11, 0, 8, 4, 4, 32, None) == 0
    build.build()
    res = build.kernel_resources()
    if res is None:
        return                                                             # (a prebuilt library: no remarks to read)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_mhatt.json")))
    mine = {k: v for k, v in res.items() if "mhatt_" in k}
    assert set(mine) == set(gold) and len(gold) == 10           # forward and query-major backward: d x tiling; key-major: d
    for kernel in ("mhatt_fwd_kernel", "mhatt_bwd_q_kernel", "mhatt_bwd_kv_kernel"):
        assert any(kernel in k for k in mine)
    assert not any("mcan_" in k for k in mine)
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0 == gold[k]["scratch"], (k, v)
        assert v.get("lds", 0) <= gold[k]["lds"] <= 65536, (k, v)


def test_the_entry_points_are_exported_and_defined_against_their_declaration():
    """what tests/test_cabi_cpu.py holds the bq_ entry points to, for the bqh_ ones: the exported bqh_ symbols are the declared
    ones, and each definition is a plain `extern "C"` in a source that sees the header through bq_common.h"""
    from bridgeqa_amd import _cabi, _ext
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ext.library_path()]).decode()
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("bqh_")}
    assert exported == set(_cabi.MHATT_PROTOS) == set(NAMES)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bridgeqa_amd", "csrc", "mhatt.hip")).read())
    assert '#include "bq_common.h"' in src and "atomic" not in src and "asm" not in src
    assert '#include "bqhip_mhatt.h"' in open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    for name in NAMES:
        heads = re.findall(r"^([^\n;{}]*?)\b%s\s*\(" % name, src, flags=re.M)
        assert heads == ['extern "C" long ' if name.endswith("ws_floats") else 'extern "C" int '], (name, heads)


def test_cpu_tensors_raise_in_the_bindings():
    from bridgeqa_amd import _ext
    q, k = torch.zeros(2, 4, 64), torch.zeros(2, 5, 64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.mhatt_fwd(q, k, k, None, None, 2)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.mhatt_bwd(q, q, k, k, torch.zeros(2, 2, 4, 5), None, None, 2)
    assert _ext.MHATT_CALLS[0] >= 0


# ---- the restatement stays inside the bounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_restatement_stays_within_the_bound(case):
    """Largest |err| / bound over all cases (fp32 restatement on the host):
        p 0.0527  out 0.0518  dq 0.0497  dk 0.0270  dv 0.257
    and exactly 0 wherever the tolerance is 0 (dv comes closest: its bound carries no term for the error of an operand)."""
    d, fwd, p32, bwd = R.reference(case)
    out, p = R.emulate_forward(d["q"], d["k"], d["v"], d["hide"], d["keep"], d["heads"])
    _ratio("p", p, fwd["p"], fwd["tol_p"])
    _ratio("out", out, fwd["out"], fwd["tol_out"])
    dq, dk, dv = R.emulate_backward(d["dout"], d["q"], d["k"], d["v"], p32, d["hide"], d["keep"], d["heads"])
    _ratio("dq", dq, bwd["dq"], bwd["tol_dq"])
    _ratio("dk", dk, bwd["dk"], bwd["tol_dk"])
    _ratio("dv", dv, bwd["dv"], bwd["tol_dv"])
    (B, heads, Nq, Nk, hd), kind, kp = case
    if kind == "mixed":
        assert (p[1] == p[1, 0, 0, 0]).all() and abs(float(p[1, 0, 0, 0]) - 1.0 / Nk) <= 2 * R.U / Nk    # uniform under a full mask
        assert (dq[1] == 0).all() and (dk[1] == 0).all()
        assert (p[0][..., d["hide"][0]] == 0).all() and (dk[0][d["hide"][0]] == 0).all() and (dv[0][d["hide"][0]] == 0).all()
    if kp:
        assert (out[0, 0, :hd] == 0).all()                                  # the query whose keep row is all zero
    if Nk == 1:
        assert (p == 1).all() and (dq == 0).all() and (dk == 0).all()
    print("worst |err| / bound so far: %s" % " ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def test_the_places_of_tolerance_zero_are_where_the_issue_puts_them():
    d, fwd, _, bwd = R.reference(((3, 3, 67, 130, 32), "mixed", True))
    hide = d["hide"]
    assert (fwd["tol_p"][0][..., hide[0]] == 0).all() and (fwd["tol_p"][0][..., ~hide[0]] > 0).all()
    assert (bwd["tol_dk"][0][hide[0]] == 0).all() and (bwd["tol_dv"][0][hide[0]] == 0).all()
    assert (bwd["tol_dq"][1] == 0).all() and (bwd["tol_dk"][1] == 0).all() and (bwd["tol_dv"][1] > 0).any()
    assert (fwd["tol_out"][0, 0, :32] == 0).all() and (fwd["tol_out"][0, 1, :32] > 0).all()


# ---- planted defects break the bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 5, 9, 32), (3, 3, 67, 130, 32), (3, 2, 70, 257, 64)])
def test_planted_defects_break_the_bound(shape):
    case = (shape, "mixed", True)
    d, fwd, p32, bwd = R.reference(case)
    args = (d["q"], d["k"], d["v"], d["hide"], d["keep"], d["heads"])
    bargs = (d["dout"], d["q"], d["k"], d["v"], p32, d["hide"], d["keep"], d["heads"])
    # no division by sqrt d: every row with more than one visible key
    out, p = R.emulate_forward(*args, defect="no_scale")
    assert _breaks(p[0], fwd["p"][0], fwd["tol_p"][0]) and _breaks(out[0], fwd["out"][0], fwd["tol_out"][0])
    # the fill as -inf: the fully hidden sample (1) is the input built for it -- NaN
    out, p = R.emulate_forward(*args, defect="fill_inf")
    assert torch.isnan(p[1]).all() and _breaks(p[1], fwd["p"][1], fwd["tol_p"][1]) and _breaks(out[1], fwd["out"][1], fwd["tol_out"][1])
    assert not _breaks(p[0], fwd["p"][0], fwd["tol_p"][0])            # a partly hidden sample does not tell the two fills apart
    # p rounded to bf16
    out, p = R.emulate_forward(*args, defect="p_bf16")
    assert _breaks(p[0], fwd["p"][0], fwd["tol_p"][0]) and _breaks(out[0], fwd["out"][0], fwd["tol_out"][0])
    # ds not zeroed under the mask: the fully hidden sample, where p is 1 / Nk and not 0
    dq, dk, _ = R.emulate_backward(*bargs, defect="no_zero")
    assert _breaks(dq[1], bwd["dq"][1], bwd["tol_dq"][1]) and _breaks(dk[1], bwd["dk"][1], bwd["tol_dk"][1])
    assert not _breaks(dq[0], bwd["dq"][0], bwd["tol_dq"][0])         # p = 0 there: the product hides the defect
    # t formed from g instead of keep g: needs a keep with zeros, sample 0 (more than one visible key)
    dq, dk, _ = R.emulate_backward(*bargs, defect="t_from_g")
    assert _breaks(dq[0], bwd["dq"][0], bwd["tol_dq"][0]) and _breaks(dk[0], bwd["dk"][0], bwd["tol_dk"][0])
    # and the restatement without a defect passes on the same input
    dq, dk, dv = R.emulate_backward(*bargs)
    assert not _breaks(dq, bwd["dq"], bwd["tol_dq"]) and not _breaks(dk, bwd["dk"], bwd["tol_dk"]) and not _breaks(dv, bwd["dv"], bwd["tol_dv"])


def test_the_reference_is_the_module_in_double():
    """the fp64 reference equals autograd of MHAtt.att run in double, keep applied as the recorded dropout multiplier"""
    case = ((3, 2, 5, 9, 32), "mixed", True)
    d, fwd, _, _ = R.reference(case)
    heads = d["heads"]
    q, k, v = [d[n].double().requires_grad_(True) for n in ("q", "k", "v")]
    m = mcan_module.MHAtt(64, num_heads=heads, pdrop=0.0).double()
    scores = torch.matmul(R.split(q, heads), R.split(k, heads).transpose(-2, -1)) / R.sqrt_d(32)
    p = torch.softmax(scores.masked_fill(d["hide"][:, None, None, :], -1e9), dim=-1)
    out = R.merge(torch.matmul(p * d["keep"].double(), R.split(v, heads)))
    assert (out.detach() - fwd["out"]).abs().max() <= 1e-12 and (p.detach() - fwd["p"]).abs().max() <= 1e-14
    out.backward(d["dout"].double())
    bwd = R.backward(d["dout"], d["q"], d["k"], d["v"], p.detach(), d["hide"], d["keep"], heads)    # p given: the exact one
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        assert (bwd[n] - t.grad).abs().max() <= 1e-11, n
    assert (q.grad[1] == 0).all() and (k.grad[1] == 0).all()                 # masked_fill passes nothing under a full mask
    assert m.head_hidden_size == 32


# ---- nothing changes with the switch off, or on the host / on ineligible inputs with it on --------------------------------------
@pytest.fixture(params=[False, True], ids=["off", "on_cpu"])
def switch(request):
    prev = mcan_module.set_fused_attention(request.param)
    yield request.param
    mcan_module.set_fused_attention(prev)


def test_the_switch_returns_the_previous_value_and_leaves_set_fused_alone():
    fused = mcan_module.fused_enabled()
    prev = mcan_module.set_fused_attention(True)
    assert mcan_module.fused_attention_enabled() is True and mcan_module.fused_enabled() is fused
    assert mcan_module.set_fused_attention(False) is True and mcan_module.fused_attention_enabled() is False
    mcan_module.set_fused_attention(prev)
    assert mcan_module.fused_attention_enabled() is prev
    before = mcan_module.set_fused(not fused)
    assert before is fused and mcan_module.fused_attention_enabled() is prev
    mcan_module.set_fused(fused)


def _grads(module, out):
    for p in module.parameters():
        p.grad = None
    out.sum().backward()
    return [p.grad.clone() for p in module.parameters()]


def test_the_blocks_are_bitwise_the_composition(switch):
    from bridgeqa_amd import _ext
    calls = list(_ext.MHATT_CALLS)
    torch.manual_seed(3)
    B, N, T, H = 3, 37, 9, 64
    x, y = torch.randn(B, N, H), torch.randn(B, T, H)
    x_mask = R.make_hide(B, N, "mixed").view(B, 1, 1, N)
    y_mask = R.make_hide(B, T, "mixed").view(B, 1, 1, T)
    att = mcan_module.MHAtt(H, num_heads=2, pdrop=0.1).train()
    full = torch.zeros(B, 1, N, T, dtype=torch.bool)                 # a per-query mask: never eligible
    full[:, :, ::3, 1] = True
    for mask in (y_mask, None, full):
        torch.manual_seed(21)
        out = att(y, y, x, mask)
        g = _grads(att, out)
        torch.manual_seed(21)
        ref = R.composition_mhatt(att, y, y, x, mask)
        g0 = _grads(att, ref)
        assert torch.equal(out, ref) and all(torch.equal(a, b) for a, b in zip(g, g0))
    sga = mcan_module.SGA(H, num_heads=2, pdrop=0.1).train()
    torch.manual_seed(11)
    out = sga(x, y, x_mask, y_mask)
    torch.manual_seed(11)
    t = sga.norm1(x, sga.dropout1(R.composition_mhatt(sga.mhatt1, x, x, x, x_mask)))
    t = sga.norm2(t, sga.dropout2(R.composition_mhatt(sga.mhatt2, y, y, t, y_mask)))
    t = sga.norm3(t, sga.dropout3(sga.ffn(t)))
    assert torch.equal(out, t)
    sa = mcan_module.SA(H, num_heads=2, pdrop=0.1).train()
    torch.manual_seed(12)
    out = sa(x, x_mask)
    torch.manual_seed(12)
    t = sa.norm1(x, sa.dropout1(R.composition_mhatt(sa.mhatt, x, x, x, x_mask)))
    t = sa.norm2(t, sa.dropout2(sa.ffn(t)))
    assert torch.equal(out, t)
    assert _ext.MHATT_CALLS == calls                                         # no host tensor ever reached a kernel


def test_ineligible_inputs_are_refused_by_the_eligibility_check():
    """what MHAtt._fused_ok looks at, on the host (the device side of it: tests/test_mhatt_gpu.py)"""
    prev = mcan_module.set_fused_attention(True)
    try:
        att = mcan_module.MHAtt(64, num_heads=2, pdrop=0.1)
        x = torch.randn(2, 5, 64)
        assert att._fused_ok(x, x, x, None) is False                                   # host tensors
        assert mcan_module.MHAtt(96, num_heads=2)._fused_ok(torch.randn(2, 5, 96), torch.randn(2, 5, 96), torch.randn(2, 5, 96), None) is False
    finally:
        mcan_module.set_fused_attention(prev)


def test_the_switch_defaults_to_off_and_the_environment_sets_it():
    code = "from bridgeqa_amd import mcan_module as m; print(int(m.fused_attention_enabled()), int(m.fused_enabled()))"
    env = {k: v for k, v in os.environ.items() if k not in ("BQ_MCAN_ATT", "BQ_MCAN_FUSED")}
    for value, want in ((None, "0 0"), ("1", "1 0"), ("0", "0 0")):
        e = dict(env, **({"BQ_MCAN_ATT": value} if value is not None else {}))
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])
