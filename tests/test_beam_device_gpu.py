"""generate's beam search on the device (csrc/beam.hip, ops.BeamState, DecodeSession.step_beams, generation.beam_search_device)
held to tests/beam_ref.py: one step on crafted logits, the ties THE ORDER of include/bqhip_beam.h settles, whole decodes on the
logits oracle (the same cases and seeds as tests/test_beam_device_cpu.py) and decodes through a model and through BLIP_VQA3D.

Decisions (selected candidates, source slots, tables, heaps, flags) are compared exactly: every case keeps a decision margin of
beam_cases.MARGIN in fp64, asserted here again for the step cases.  Candidate scores are held to err <= K E32 + ULP
(beam_cases.K, fixed from a CPU emulation before any device run)."""
import numpy as np
import pytest
import torch

import beam_cases as C
import beam_ref as R

pytestmark = pytest.mark.gpu


# ---- a BeamState filled from a reference state ------------------------------------------------------------------------------------
def device_state(p, st, dev):
    from bridgeqa_amd import fusion_ops as ops
    S, nb, ML = p["B"] * p["nb"], p["nb"], p["max_length"]
    cache = ops.DecodeCache(0, S, st["anc"].shape[0], 1, dev)
    prompt = torch.full((S, 1), C.BOS, dtype=torch.long, device=dev)
    bs = ops.BeamState(cache, prompt, nb, ML, p["eos"], p["pad"], min_length=p["min_length"], length_penalty=p["length_penalty"],
                       early_stopping=p["early_stopping"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    bs.beam_score.copy_(t(st["beam_score"], torch.float32))
    bs.tokens.copy_(t(st["tokens"], torch.int32))
    bs.done.copy_(t(st["done"], torch.int32))
    bs.ids.copy_(t(st["ids"], torch.int64)[:, None])
    cache.anc.copy_(t(st["anc"], torch.int32))
    cache.t = st["cur_len"] - 1
    cache.pos.fill_(cache.t)
    for b, h in enumerate(st["heaps"]):
        n = len(h.beams)
        bs.heap_len[b], bs.heap_adds[b], bs.heap_worst[b] = n, n, h.worst
        for i, (score, toks, s32) in enumerate(h.beams):
            bs.heap_seq[b, i], bs.heap_hyplen[b, i], bs.heap_sum[b, i], bs.heap_score[b, i] = i, len(toks), float(s32), score
            bs.heap_tokens[b, i, :len(toks)] = torch.tensor(toks, dtype=torch.int32)
    return cache, bs


def run_step(cache, bs, logits):
    """what DecodeSession.step_beams does after the decoder forward"""
    cache.advance()
    bs.step(logits)
    torch.cuda.synchronize()


def check_against_reference(p, ref, rec, cache, bs, cur_len):
    """ref: the reference state AFTER the step, rec: what the reference step returned; cur_len: of the step"""
    h = bs.host()
    B, nb = p["B"], p["nb"]
    live = ~np.asarray([bool(d) for d in ref["done_before"]])
    assert h["top_index"].numpy()[live].tolist() == rec["top_index"][live].tolist()     # (a done sample's are not used)
    assert h["src"].numpy().tolist() == rec["src"].tolist()
    assert h["tokens"].numpy()[:, :cur_len + 1].tolist() == ref["tokens"][:, :cur_len + 1].tolist()
    assert cache.anc.cpu().numpy().tolist() == ref["anc"].tolist()
    assert bs.ids.cpu().numpy()[:, 0].tolist() == ref["ids"].tolist()
    assert h["done"].numpy().astype(bool).tolist() == ref["done"].tolist()
    assert int(h["not_done"][0]) == rec["not_done"] == int(h["not_done"][1 + cur_len])
    assert int(cache.pos) == cur_len == cache.t
    hyps, _ = bs.hypotheses(h)
    lp = R.lenpow_table(p["max_length"], p["length_penalty"])
    for b in range(B):
        want = ref["heaps"][b]
        assert len(hyps[b].beams) == len(want.beams) == int(h["heap_len"][b])
        assert [toks for _, toks in hyps[b].beams] == [toks for _, toks, _ in want.beams]
        got = [float(h["heap_score"][b, i]) for i in range(int(h["heap_len"][b]))]
        for i, g in enumerate(got):                 # the heap's arithmetic is exact: double(sum_logprobs) / lenpow[len]
            assert _same(g, float(h["heap_sum"][b, i]) / lp[int(h["heap_hyplen"][b, i])])
        if got and not np.isnan(got).any():
            assert float(h["heap_worst"][b]) == min(got)
        assert np.allclose([s for s, _ in hyps[b].beams], [s for s, _, _ in want.beams], rtol=0, atol=1e-5, equal_nan=True)
    assert np.array_equal(h["beam_score"].numpy()[np.repeat(~live, nb)], np.zeros(int((~live).sum()) * nb, np.float32))
    return h


def _same(a, b):
    return a == b or (a != a and b != b)


def score_bound(p, h, st_before, logits32, cur_len):
    """the step's 2 nb candidate scores per sample against fp64: err <= K E32 + ULP"""
    nb, V = p["nb"], p["V"]
    idx = h["top_index"].numpy().astype(np.int64)                                  # (B, 2 nb) flat r_local V + v
    rows = np.arange(p["B"])[:, None] * nb + idx // V
    err, e32, ulp = R.score_errors(h["top_score"].numpy(), logits32, st_before["beam_score"], cur_len, p, index=(rows, idx % V))
    closed = np.abs(st_before["beam_score"][rows]) > 1e8                            # step 0: -1e9 + x is -1e9, one ulp is 64
    fin = np.isfinite(err) & ~closed
    worst = float(err[fin].max()) if fin.any() else 0.0
    print("candidate scores: worst error %.3e, E32 %.3e, ULP %.3e, bound %.3e" % (worst, e32, ulp, C.K * e32 + ulp))
    assert worst <= C.K * e32 + ulp
    return worst


def copy_state(st):
    out = dict(st)
    for k in ("beam_score", "tokens", "anc", "done", "ids"):
        out[k] = st[k].copy()
    out["heaps"] = []
    for h in st["heaps"]:
        g = R.Heap(h.nb, h.lenpow, h.early)
        g.beams, g.worst = list(h.beams), h.worst
        out["heaps"].append(g)
    return out


def one_step(p, st, logits32, dev, dtype=torch.float32, misalign=False):
    """the device step and the reference step from the same state; returns (host copy of the device state, margins)"""
    before = copy_state(st)
    cache, bs = device_state(p, st, dev)
    lg = torch.from_numpy(np.ascontiguousarray(logits32)).to(dev).to(dtype)
    if misalign:                                        # rows that start off a 16-byte boundary even for an even V
        buf = torch.zeros(lg.numel() + 1, dtype=dtype, device=dev)
        buf[1:].copy_(lg.reshape(-1))
        lg = buf[1:].view(lg.shape)
    cur_len = st["cur_len"]
    run_step(cache, bs, lg)
    margins = []
    ref = copy_state(st)
    rec = R.step(ref, logits32, p, margins)
    ref["done_before"] = before["done"]
    h = check_against_reference(p, ref, rec, cache, bs, cur_len)
    return h, before, margins, cur_len


@pytest.mark.parametrize("case", C.step_cases(), ids=C.step_id)
def test_one_step_against_the_reference(case, dev):
    from bridgeqa_amd import _ext
    p, st, logits = C.make_step(case)
    calls = _ext.BEAM_CALLS[0]
    h, before, margins, cur_len = one_step(p, st, logits, dev, torch.bfloat16 if case[5] == "bf16" else torch.float32)
    assert _ext.BEAM_CALLS[0] == calls + 1
    low = min([v for _, v in margins if not (case[5] == "bf16" and v == 0.0)] or [np.inf])
    assert low >= C.MARGIN, low
    score_bound(p, h, before, logits, cur_len)


def test_rows_off_a_16_byte_boundary(dev):
    for case in ((3, 10, 200, 1, False, "f32"), (3, 10, 200, 1, True, "bf16")):
        p, st, logits = C.make_step(case)
        one_step(p, st, logits, dev, torch.bfloat16 if case[5] == "bf16" else torch.float32, misalign=True)


# ---- ties: THE ORDER decides, the reference's own rule is the yardstick ------------------------------------------------------------
def test_a_row_of_equal_logits(dev):
    p, st, logits = C.make_step((3, 5, 33, 1, False, "f32"))
    logits, st["beam_score"] = logits.copy(), st["beam_score"].copy()
    logits[0] = 0.0                       # beam 0 of sample 0: 33 equal scores ...
    st["beam_score"][0] += np.float32(4.0)  # ... ahead of every other beam: the lowest token indices win, in order
    logits[12] = 1.5                      # and a whole row of sample 2, wherever its beam stands
    h, _, _, _ = one_step(p, st, logits, dev)
    assert h["top_index"].numpy()[0].tolist() == list(range(10))


def test_two_beams_whose_scores_collide(dev):
    """equal beam scores over equal rows: every candidate of beam 1 ties with beam 0's -- the flat index interleaves them"""
    p, st, logits = C.make_step((3, 5, 33, 1, False, "f32"))
    logits, st["beam_score"] = logits.copy(), st["beam_score"].copy()
    logits[1] = logits[0]
    st["beam_score"][1] = st["beam_score"][0]
    h, _, _, _ = one_step(p, st, logits, dev)
    idx = h["top_index"].numpy()[0].tolist()
    firsts = [j for j, f in enumerate(idx[:-1]) if f < p["V"]]
    assert firsts and all(idx[j + 1] == idx[j] + p["V"] for j in firsts)       # beam 1's same token right behind beam 0's


@pytest.mark.parametrize("nb,V", [(5, 11), (5, 10), (16, 33), (1, 3)])
def test_the_closed_beams_of_step_0_collide_at_minus_1e9(nb, V, dev):
    """eos suppressed: beam 0 has V - 1 finite candidates, every candidate of beams 1 .. nb - 1 rounds to -1e9.  V = 2 nb + 1
    fills the 2 nb ranks from beam 0; V = 2 nb (the entry point's own limit) reaches INTO the collision at the last rank, where
    the index rule must pick the first token of beam 1"""
    p = C.step_params(2, nb, V, C.STEP_MAX_LENGTH)
    st, logits = C.state_at(p, 0)
    h, _, _, _ = one_step(p, st, logits, dev)
    idx = h["top_index"].numpy()
    if V == 2 * nb:
        assert (idx[:, -1] == V).all() and (idx[:, :-1] < V).all()
        assert (h["top_score"].numpy()[:, -1] == np.float32(-1e9)).all()
    else:
        assert (idx < V).all()


def test_a_nan_logit_ranks_first_and_nothing_faults(dev):
    """log_softmax of a row with a NaN is NaN everywhere: the row's candidates rank first in index order"""
    p, st, logits = C.make_step((3, 5, 33, 1, False, "f32"))
    logits = logits.copy()
    logits[3, 17] = np.nan                # sample 0, beam 3
    h, _, _, _ = one_step(p, st, logits, dev)
    idx, sc = h["top_index"].numpy()[0], h["top_score"].numpy()[0]
    assert idx.tolist() == list(range(3 * 33, 3 * 33 + 10)) and np.isnan(sc).all()
    assert np.isnan(h["beam_score"].numpy()[:5]).all() and np.isfinite(h["beam_score"].numpy()[10:]).all()


def test_bad_extents_are_refused_before_any_launch(dev):
    from bridgeqa_amd import fusion_ops as ops
    p = C.step_params(1, 5, 9, 0)
    cache = ops.DecodeCache(0, 5, 8, 1, dev)
    bs = ops.BeamState(cache, torch.full((5, 1), C.BOS, dtype=torch.long, device=dev), 5, 8, p["eos"], p["pad"])
    cache.advance()
    with pytest.raises(RuntimeError, match="bad extents"):
        bs.step(torch.zeros(5, 9, device=dev))                       # V < 2 nb
    with pytest.raises(RuntimeError, match="logits"):
        bs.step(torch.zeros(5, 33, dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="CPU"):
        bs.step(torch.zeros(5, 33))


# ---- whole decodes on the oracle --------------------------------------------------------------------------------------------------
class OracleSession(object):
    """step_beams() as DecodeSession's, with the oracle in place of the decoder: logits from the device tables, then the
    position increment and the beam kernels"""

    def __init__(self, p, dev):
        from bridgeqa_amd import fusion_ops as ops
        S = p["B"] * p["nb"]
        orc = R.make_oracle(p)
        self.A, self.C = torch.from_numpy(orc["A"]).to(dev), torch.from_numpy(orc["C"]).to(dev)
        self.sample = torch.arange(S, device=dev) // p["nb"]
        self.cache = ops.DecodeCache(0, S, p["max_length"], 1, dev)
        self.state = ops.BeamState(self.cache, torch.full((S, 1), C.BOS, dtype=torch.long, device=dev), p["nb"], p["max_length"],
                                   p["eos"], p["pad"], min_length=p["min_length"], length_penalty=p["length_penalty"],
                                   early_stopping=p["early_stopping"])
        self.steps = 0

    def step_beams(self):
        logits = self.A[self.cache.t, self.sample] + self.C[self.state.ids[:, 0] % 64]
        self.cache.advance()
        self.state.step(logits)
        self.steps += 1


def device_decode(p, dev, stop_lag=1):
    from bridgeqa_amd.generation import beam_search_device
    s = OracleSession(p, dev)
    seq, scores = beam_search_device(s, s.state, stop_lag=stop_lag)
    return seq.cpu().numpy(), scores.cpu().numpy(), s.steps


@pytest.fixture(scope="module")
def reference_runs():
    return {C.case_id(p): C.run_case(p) for p in C.decode_cases()}


@pytest.mark.parametrize("p", C.decode_cases(), ids=C.case_id)
def test_whole_decode_on_the_oracle(p, dev, reference_runs):
    r = reference_runs[C.case_id(p)]
    seq, scores, steps = device_decode(p, dev)
    assert seq.tolist() == r["seq"].tolist()
    assert float(np.abs(scores.astype(np.float64) - r["scores"]).max()) <= 1e-5
    assert r["steps"] <= steps <= min(r["steps"] + 1, p["max_length"] - 1)      # the stop check lags one step


def test_steps_after_all_done_change_nothing(dev, reference_runs):
    """the stop check forced to see `all done` at once (0 extra steps), one step late (1) and never (all remaining steps)"""
    early = [p for p in C.decode_cases() if reference_runs[C.case_id(p)]["all_done"]]
    assert len(early) >= 3
    for p in early:
        r = reference_runs[C.case_id(p)]
        want = {0: r["steps"], 1: min(r["steps"] + 1, p["max_length"] - 1), None: p["max_length"] - 1}
        for lag in (0, 1, None):
            seq, scores, steps = device_decode(p, dev, stop_lag=lag)
            assert steps == want[lag], (C.case_id(p), lag, steps)
            assert seq.tolist() == r["seq"].tolist()
            assert float(np.abs(scores.astype(np.float64) - r["scores"]).max()) <= 1e-5


def test_the_kinds_of_decode_are_all_there(reference_runs):
    for what in ("all_done", "mixed", "evicted", "ignored_eos"):
        assert any(r[what] for r in reference_runs.values()), what


# ---- through a model ------------------------------------------------------------------------------------------------------------
# MSEED: the first device run measured the host route's margins of seeds 0 .. 119 (34 keep 1e-4); 69 has the widest (3.2e-3) and
# one sample that finishes early beside two that run out.  bf16 logits repeat inside a row, so most seeds hold an exact tie
MV, MB, MNB, MLEN, MSEED = 200, 3, 5, 8, 69
BLIP_SEED = 0
# the early-finish model: of the first five seeds per eos bias that keep the margin (first device run), the one that decodes
# more than one token before it ends
ESEED, EBIAS, EMLEN = 17, 6.0, 16


class _dtype(object):
    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        from bridgeqa_amd import fusion_ops as ops
        self.prev = ops.set_compute_dtype(self.dt)

    def __exit__(self, *a):
        from bridgeqa_amd import fusion_ops as ops
        ops.set_compute_dtype(self.prev)


def make_model(dev, seed=MSEED, vocab=MV, max_positions=80, eos_bias=3.0):
    from bridgeqa_amd import med
    cfg = med.BertConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, vocab_size=vocab,
                         max_position_embeddings=max_positions, encoder_width=128)
    torch.manual_seed(seed)
    dec = med.BertLMHeadModel(config=cfg).to(dev).eval()
    with torch.no_grad():
        dec.cls.predictions.bias.copy_(torch.randn(vocab, device=dev) * 1.5)
        dec.cls.predictions.bias[C.EOS] += eos_bias
        dec.cls.predictions.bias.sub_(4.0)      # (log-softmax does not see a shift: the top logits come to lie around 0, where
        dec.cls.predictions.decoder.weight.mul_(8.0)   # bf16 is finest, so fewer of them coincide)
    return dec


def model_inputs(dev, nb=MNB, B=MB, prompt=(C.BOS,), seed=21):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B * nb, 7, 128, generator=g).to(dev)
    m = torch.ones(B, 7, dtype=torch.long)
    m[1, 4:] = 0                                        # ragged: sample 1 sees 4 of its 7 encoder tokens
    m[B - 1, 6:] = 0
    ids = torch.tensor([list(prompt)] * B, dtype=torch.long, device=dev)
    return ids, dict(encoder_hidden_states=enc, encoder_attention_mask=m.repeat_interleave(nb, dim=0).to(dev))


class record_host_steps(object):
    """the logits every DecodeSession.step returns while the block runs: what the host route's search saw"""

    def __enter__(self):
        from bridgeqa_amd import med
        self.seen, self.orig = [], med.DecodeSession.step
        rec = self

        def step(session, ids):
            logits = rec.orig(session, ids)
            rec.seen.append(logits.float().cpu().numpy())
            return logits
        med.DecodeSession.step = step
        return self

    def __exit__(self, *a):
        from bridgeqa_amd import med
        med.DecodeSession.step = self.orig


def host_route_margin(seen, nb, max_length, min_length, eos, pad):
    """the reference over the host route's own step logits -> (its smallest decision margin, its sequences).  bf16 logits
    repeat inside a row, and what torch.topk does with equal scores is not promised: an exact tie counts as margin 0 here"""
    p = dict(B=seen[0].shape[0] // nb, nb=nb, V=seen[0].shape[1], max_length=max_length, min_length=min_length,
             length_penalty=1.0, early_stopping=False, eos=eos, pad=pad)
    st, margins = R.new_state(p), []
    for lg in seen:
        if st["done"].all():
            break
        R.step(st, lg, p, margins)
    return min(v for _, v in margins), R.finalize(st, p)[0]


@pytest.fixture(scope="module")
def model(dev):
    return make_model(dev)


def test_generate_through_a_model(model, dev):
    from bridgeqa_amd import _ext, med
    ids, kw = model_inputs(dev)
    gen = dict(max_length=MLEN, min_length=1, num_beams=MNB)
    with _dtype(torch.bfloat16):
        args = dict(eos_token_id=C.EOS, pad_token_id=C.PAD, return_scores=True, **gen, **kw)
        with record_host_steps() as rec:
            host = model.generate(ids, device_beams=False, graph=True, **args)
        margin, ref_seq = host_route_margin(rec.seen, MNB, MLEN, 1, C.EOS, C.PAD)
        print("host route: smallest decision margin %.3e over %d steps" % (margin, len(rec.seen)))
        assert margin >= C.MARGIN
        assert ref_seq.tolist() == host[0].cpu().numpy().tolist()
        for graph in (False, True):
            stats, calls, dcalls = dict(med._DECODE_STATS), _ext.BEAM_CALLS[0], list(_ext.DECODE_CALLS)
            a = model.generate(ids, device_beams=True, graph=graph, **args)
            steps = _ext.BEAM_CALLS[0] - calls
            assert med._DECODE_STATS["beam_steps"] - stats["beam_steps"] == MLEN - 1        # a sample runs out: every step
            assert med._DECODE_STATS["beam_decodes"] == stats["beam_decodes"] + 1
            assert med._DECODE_STATS["sessions"] == stats["sessions"] + 1
            assert med._DECODE_STATS["captures"] - stats["captures"] == (1 if graph else 0)        # exactly one graph
            assert med._DECODE_STATS["beam_captures"] - stats["beam_captures"] == (1 if graph else 0)
            # eager: one call of the entry point per step; graph: the first step's and the captured one's
            assert (steps == 2) if graph else (1 <= steps <= MLEN - 1)
            assert _ext.DECODE_CALLS[0] > dcalls[0] and _ext.DECODE_CALLS[0] - dcalls[0] == _ext.DECODE_CALLS[1] - dcalls[1]
            assert torch.equal(a[0], host[0]), (a[0], host[0])
            assert float((a[1] - host[1]).abs().max()) <= 1e-5
            b = model.generate(ids, device_beams=True, graph=graph, **args)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))     # the same bits


def test_a_model_whose_samples_all_finish_stops_the_replays_early(dev):
    """the stop check of the graph route: every sample is done after a few steps, the loop sees it one step late and the result
    is the host route's"""
    from bridgeqa_amd import med
    dec = make_model(dev, seed=ESEED, eos_bias=EBIAS)
    ids, kw = model_inputs(dev)
    args = dict(eos_token_id=C.EOS, pad_token_id=C.PAD, return_scores=True, max_length=EMLEN, min_length=1, num_beams=MNB, **kw)
    with _dtype(torch.bfloat16):
        with record_host_steps() as rec:
            host = dec.generate(ids, device_beams=False, graph=True, **args)
        margin, ref_seq = host_route_margin(rec.seen, MNB, EMLEN, 1, C.EOS, C.PAD)
        print("host route: smallest decision margin %.3e, all done after %d of %d steps" % (margin, len(rec.seen), EMLEN - 1))
        assert margin >= C.MARGIN and len(rec.seen) <= EMLEN - 3
        assert ref_seq.tolist() == host[0].cpu().numpy().tolist()
        for graph in (False, True):
            steps = med._DECODE_STATS["beam_steps"]
            a = dec.generate(ids, device_beams=True, graph=graph, **args)
            assert med._DECODE_STATS["beam_steps"] - steps == len(rec.seen) + 1          # one step late, not max_length - 1
            assert torch.equal(a[0], host[0]) and float((a[1] - host[1]).abs().max()) <= 1e-5


def test_switch_off_runs_nothing_of_the_route(model, dev):
    from bridgeqa_amd import _ext, med
    prev, med._BEAM_DEVICE[0] = med._BEAM_DEVICE[0], False           # (whatever the environment of this run says)
    ids, kw = model_inputs(dev)
    with _dtype(torch.bfloat16):
        stats, calls, dcalls = dict(med._DECODE_STATS), _ext.BEAM_CALLS[0], list(_ext.DECODE_CALLS)
        model.generate(ids, max_length=MLEN, min_length=1, num_beams=MNB, eos_token_id=C.EOS, pad_token_id=C.PAD, **kw)
        assert _ext.BEAM_CALLS[0] == calls
        assert med._DECODE_STATS["beam_decodes"] == stats["beam_decodes"] and med._DECODE_STATS["beam_captures"] == stats["beam_captures"]
        assert med._DECODE_STATS["sessions"] == stats["sessions"] + 1 and _ext.DECODE_CALLS[0] > dcalls[0]
    med._BEAM_DEVICE[0] = prev


INELIGIBLE = [("17 beams", 200, 17, 6, (C.BOS,)), ("V = 2 nb", 10, 5, 6, (C.BOS,)), ("max_length 65", 200, 2, 65, (C.BOS,)),
              ("a prompt of two tokens", 200, 4, 6, (C.BOS, 7))]


@pytest.mark.parametrize("why,vocab,nb,max_length,prompt", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_decodes_take_todays_path(why, vocab, nb, max_length, prompt, dev):
    from bridgeqa_amd import _ext, med
    dec = make_model(dev, vocab=vocab)
    ids, kw = model_inputs(dev, nb=nb, B=2, prompt=prompt)
    args = dict(max_length=max_length, min_length=1, num_beams=nb, eos_token_id=C.EOS, pad_token_id=C.PAD, return_scores=True, **kw)
    with _dtype(torch.bfloat16):
        off = dec.generate(ids, device_beams=False, **args)
        calls, decodes = _ext.BEAM_CALLS[0], med._DECODE_STATS["beam_decodes"]
        on = dec.generate(ids, device_beams=True, **args)
    assert _ext.BEAM_CALLS[0] == calls and med._DECODE_STATS["beam_decodes"] == decodes
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_fp32_compute_dtype_takes_todays_path(model, dev):
    from bridgeqa_amd import _ext
    ids, kw = model_inputs(dev)
    args = dict(max_length=6, min_length=1, num_beams=MNB, eos_token_id=C.EOS, pad_token_id=C.PAD, return_scores=True, **kw)
    with _dtype(torch.float32):
        off = model.generate(ids, device_beams=False, **args)
        calls = _ext.BEAM_CALLS[0]
        on = model.generate(ids, device_beams=True, **args)
    assert _ext.BEAM_CALLS[0] == calls and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def blip_rig(dev, seed):
    """BLIP_VQA3D on the golden inputs of tests/test_generate_cpu.run_blip_generate -> a function returning its answers"""
    import os
    import conftest
    from bridgeqa_amd import med
    from bridgeqa_amd.blip_vqa_3d import BLIP_VQA3D, SyntheticTokenizer
    from golden_util import fill_params
    cfg = med.BertConfig(num_hidden_layers=2, vocab_size=200, max_position_embeddings=64)
    m = BLIP_VQA3D(med_config=cfg, image_size=64, num_answers=10, use_text_decoder=True, share_decoder=True, scene_size=32,
                   tokenizer=SyntheticTokenizer(0, 102, 198, 199))
    fill_params(m, "blip_model.")
    m = m.to(dev).eval()
    head = m.text_decoder.cls.predictions            # the fixture's logits are nearly flat: sharpen them, as make_model does,
    with torch.no_grad():                            # so that the search has decisions to take rather than ties
        head.bias.copy_(torch.randn(200, generator=torch.Generator().manual_seed(seed)).to(dev) * 1.5)
        head.decoder.weight.mul_(8.0)
    gm = dict(np.load(os.path.join(conftest.GOLDEN, "fusion_med.npz")))
    gb = dict(np.load(os.path.join(conftest.GOLDEN, "fusion_blip.npz")))
    t = lambda g_, k: torch.from_numpy(g_[k]).to(dev)
    q = {"input_ids": t(gm, "tw_ids"), "attention_mask": t(gm, "tw_am")}

    def answers():
        with torch.no_grad():
            return m(t(gb, "bl_img"), q, None, train=False, inference="generate", scene_object_embeds=t(gb, "bl_obj"),
                     scene_object_mask=t(gm, "tw_om"), data_dict={})[0]
    return answers, q["input_ids"].shape[0]


def test_blip_vqa3d_generate_with_the_switch_on(dev):
    """BLIP_VQA3D.forward(inference='generate') needs nothing beyond the switch: the answers of the host route.  Ten beams over 19
    steps of bf16 logits always hold exact ties somewhere (the margin printed below is 0 for every head seed tried), so unlike
    test_generate_through_a_model this comparison rests on torch.topk returning equal scores in index order, as it did for all
    six head seeds of the first device run"""
    from bridgeqa_amd import _ext, med
    answers, n = blip_rig(dev, BLIP_SEED)
    prev = med._BEAM_DEVICE[0]
    with _dtype(torch.bfloat16):
        try:
            med._BEAM_DEVICE[0] = False
            calls, decodes = _ext.BEAM_CALLS[0], med._DECODE_STATS["beam_decodes"]
            with record_host_steps() as rec:
                off = answers()
            assert _ext.BEAM_CALLS[0] == calls and med._DECODE_STATS["beam_decodes"] == decodes
            margin, _ = host_route_margin(rec.seen, 10, 20, 1, 102, 0)
            print("host route: smallest decision margin %.3e over %d steps" % (margin, len(rec.seen)))
            med._BEAM_DEVICE[0] = True
            on = answers()
            assert med._DECODE_STATS["beam_decodes"] == decodes + 1 and _ext.BEAM_CALLS[0] > calls
        finally:
            med._BEAM_DEVICE[0] = prev
    assert len(on) == n and on == off
