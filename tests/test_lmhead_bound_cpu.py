"""The per-row / per-element bound of tests/lmhead_ref.py, checked without a GPU: an fp32 emulation of the LM-head kernels'
arithmetic stays well inside it at every shape of the battery and every smoothing, and each planted defect -- applied inside
the emulation at a shape where it can act -- is rejected by it, most of them where the whole-tensor norms of
tests/test_gemm_gpu.py::test_lm_head_cross_entropy_vs_torch accept them."""
import pytest
import torch

import lmhead_ref as R


def _ratio(out, ref, tol):
    r, msg = R.excess(out, ref, tol)
    assert msg is None, msg
    return r


def _rejected(out, ref, tol):
    return R.excess(out, ref, tol)[1] is not None


def _case_id(c):
    return "R%d-D%d-V%d%s" % (c[0], c[1], c[2], "-shift%+g" % c[3] if c[3] else "")


def _run(case, eps, defect=None, chained=False):
    """the emulation's outputs and the references they are held to, as {kind: (out, ref, tol)}.  dlogits takes the test-made
    logits and lse (chained: the emulation's own forward outputs, as the GPU suite's second way)."""
    Rr, D, V, shift = case
    d, f = R.inputs(*case), R.forward_of(*case)
    x, ls, lse, z32 = R.emulate_forward(d["h"], d["w"], d["bias_pad"], d["tgt"], V, eps, defect)
    loss, tol_loss, _ = R.loss(f, d["tgt"], eps)
    xin, lin = (x, lse) if chained else R.made_forward_outputs(f, V)
    dl, dl32 = R.emulate_dlogits(xin, lin, d["g"], d["tgt"], V, eps, defect)
    dref, dtol, e_d = R.dlogits(xin, lin, d["g"], d["tgt"], V, eps)
    return dict(logits=(x[:, :V], f["z"], f["tol_x"]), pad=x[:, V:], lse=(lse, f["L"], f["tol_L"]), loss=(ls, loss, tol_loss),
                dlogits=(dl, dref, dtol), logits32=(z32[:, :V], f["z"], f["e_z"]), dlogits32=(dl32, dref, e_d))


@pytest.mark.parametrize("eps", R.SMOOTHINGS)
@pytest.mark.parametrize("case", R.CASES, ids=_case_id)
def test_emulation_stays_within_half_the_bound(case, eps):
    """|err| / tol <= 0.5 for the fp32 outputs lse and loss, and for the two bf16 outputs taken BEFORE their one rounding: the
    bound is not tighter than the arithmetic.  Those unrounded values are also held to the fp32 part (e_z, e_d) of their
    tolerance alone, <= 1 (the exponent term 3 u |x - l| of e_d covers two roundings and the exponential: it has no factor two to
    give).  The ROUNDED bf16 outputs are held to <= 1: a correct round-to-nearest just above a power of two errs by 2^-8
    relative, which is the whole of the tolerance 2^-8 |r| (0.99 is reached here), so no rounded result can leave a factor two.
    Largest ratios over the battery: lse 0.027, loss 0.030, unrounded logits 0.15 of e_z (0.0014 of the whole tolerance),
    unrounded dlogits 0.58 of e_d (0.09 of the whole tolerance)."""
    o = _run(case, eps)
    worst = {k: _ratio(*o[k]) for k in ("logits", "lse", "loss", "dlogits", "logits32", "dlogits32")}
    worst["logits32/tol"] = _ratio(o["logits32"][0], o["logits"][1], o["logits"][2])
    worst["dlogits32/tol"] = _ratio(o["dlogits32"][0], o["dlogits"][1], o["dlogits"][2])
    assert not bool(o["pad"].float().any()), "padding columns of the logits"
    print("%s eps=%g largest |err| / bound: %s" % (_case_id(case), eps, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(worst[k] <= 0.5 for k in ("lse", "loss", "logits32/tol", "dlogits32/tol")), worst
    assert all(worst[k] <= 1.0 for k in ("logits", "dlogits", "logits32", "dlogits32")), worst


def test_chained_dlogits_emulation_stays_within_the_bound():
    o = _run(R.CASES[1], 0.1, chained=True)
    assert _ratio(*o["dlogits32"]) <= 1.0 and _ratio(*o["dlogits"]) <= 1.0


def test_ignored_rows_and_padding_are_exact_zeros_in_reference_and_emulation():
    case = R.CASES[1]
    d = R.inputs(*case)
    o = _run(case, 0.1)
    ign = d["tgt"] < 0
    assert bool(ign.any()) and not bool(ign.all()) and int(d["tgt"][-1]) >= 0
    for out, ref, tol in (o["loss"], o["dlogits"]):
        assert bool((ref[ign] == 0).all()) and bool((tol[ign] == 0).all()) and bool((out.float()[ign] == 0).all())
    dl, dref, dtol = o["dlogits"]
    assert bool((dref[:, case[2]:] == 0).all()) and bool((dtol[:, case[2]:] == 0).all()) and not bool(dl[:, case[2]:].float().any())
    # where the tolerance is 0 anything else fails
    bad = o["loss"][0].clone()
    bad[ign.nonzero()[0, 0]] = 1e-30
    assert _rejected(bad, o["loss"][1], o["loss"][2])


def test_the_inputs_hold_the_rows_the_battery_is_about():
    for case in R.CASES:
        Rr, D, V, shift = case
        d, f = R.inputs(*case), R.forward_of(*case)
        tg = d["tgt"]
        valid = [int(t) for t in tg if t >= 0]
        assert int(tg[-1]) >= 0 and bool((tg < 0).any()) and all(0 <= t < V for t in valid)
        assert V - 1 in valid and 0 in valid
        span = float(f["z"][1].amax() - f["z"][1].amin())
        assert span > 60.0, span                                        # row 1: a logit range the max subtraction must carry
        assert bool((d["g"] > 0).all())
        if Rr >= 18:
            assert any(int(tg[r]) == int(f["z"][r].argmax()) for r in range(Rr))
            assert all(t in valid for t in (127, 128, 255, 256) if t < V)
    assert R.n_records(100) == 2 and R.padded(100) == 128 and R.n_records(8200) == 66 and R.n_records(30524) == 240
    # without the max subtraction fp32 overflows at +90 (every row: inf); at -90 most exponentials are below the normal range
    # (lost to a flush to zero), though their sum of 200 -- 2e-37 -- is still a normal number here
    up, down = (R.forward_of(*(R.SHIFT_SHAPE + (s,)))["z"].float() for s in R.SHIFTS)
    assert bool(torch.isinf(torch.exp(up).sum(1)).all())
    assert float((torch.exp(down) < R.TINY).double().mean()) > 0.5


# ---- planted defects ------------------------------------------------------------------------------------------------------------
TINY_CASE = (18, 256, 200, 0.0)     # today's tiny shape: three sequences of six rows
EMPTY_HALF = (5, 64, 100, 0.0)
MANY_RECORDS = (3, 64, 8200, 0.0)


def _accepts(o, seq):
    """the restated old norms on the three outputs they can see"""
    return (R.old_norms_accept("logits", o["logits"][0], o["logits"][1]) and R.old_norms_accept("loss", o["loss"][0], o["loss"][1], seq)
            and R.old_norms_accept("dlogits", o["dlogits"][0], o["dlogits"][1]))


@pytest.mark.parametrize("case,seq", [(TINY_CASE, 6), (EMPTY_HALF, 5), (MANY_RECORDS, 3)], ids=lambda v: _case_id(v) if isinstance(v, tuple) else "")
def test_the_clean_emulation_passes_norms_and_bound(case, seq):
    o = _run(case, 0.1)
    assert _accepts(o, seq)
    assert not any(_rejected(*o[k]) for k in ("logits", "lse", "loss", "dlogits"))


@pytest.mark.parametrize("case,seq", [(EMPTY_HALF, 5), (TINY_CASE, 6)], ids=lambda v: _case_id(v) if isinstance(v, tuple) else "")
def test_defect_a_target_logit_taken_from_the_bf16_store(case, seq):
    o = _run(case, 0.1, "zt_from_bf16")
    assert _accepts(o, seq)                                   # old norms: accepted (about 2e-4 of the largest loss)
    assert _rejected(*o["loss"])
    assert not _rejected(*o["lse"]) and not _rejected(*o["logits"])


def test_defect_b_statistics_without_the_last_vocabulary_entry():
    o = _run(TINY_CASE, 0.1, "stats_skip_last")
    assert _rejected(*o["lse"]) and _rejected(*o["loss"])
    # the row whose target is V - 1 loses its target logit altogether, which the old loss norm does see: not accepted
    assert not R.old_norms_accept("loss", o["loss"][0], o["loss"][1], 6)
    rows = R.inputs(*TINY_CASE)["tgt"] != TINY_CASE[2] - 1
    assert R.old_norms_accept("loss", o["loss"][0][rows], o["loss"][1][rows])      # ... but nothing on the other rows
    assert _rejected(o["lse"][0][rows], o["lse"][1][rows], o["lse"][2][rows])


@pytest.mark.parametrize("eps,old_accept", [(0.1, True), (0.3, False)])
def test_defect_c_smoothing_term_missing_from_dlogits(eps, old_accept):
    o = _run(TINY_CASE, eps, "no_smoothing_term")
    assert _accepts(o, 6) == old_accept                       # old norms: its L2 weight is eps^2 / V -- accepted at the 0.1 they ran
    assert _rejected(*o["dlogits"])


def test_defect_d_merge_keeps_the_stale_maximum():
    o = _run(TINY_CASE, 0.1, "stale_max")
    assert _rejected(*o["lse"]) and _rejected(*o["loss"])
    assert not R.old_norms_accept("loss", o["loss"][0], o["loss"][1], 6)           # (a whole maximum off: the old norm sees it)


def test_defect_e_combine_reads_only_the_first_64_records():
    """the last 8 of 8200 entries never reach lse or the mean logit"""
    o = _run(MANY_RECORDS, 0.1, "first_64_records")
    assert _accepts(o, 3)                                     # old norms: accepted
    assert _rejected(*o["lse"]) and _rejected(*o["loss"])


def test_defect_f_empty_half_tile_merged_without_its_guard_is_nan_and_fails():
    o = _run(EMPTY_HALF, 0.1, "no_inf_guard")
    assert bool(torch.isnan(o["lse"][0]).any())
    ratio, msg = R.excess(*o["lse"])
    assert msg is not None and ratio == float("inf")
    assert _rejected(*o["loss"])
    assert not R.old_norms_accept("loss", o["loss"][0], o["loss"][1], 5)
