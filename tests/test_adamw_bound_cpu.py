"""The per-element bound of tests/adamw_ref.py, checked without a GPU: an fp32 emulation of adamw_kernel's arithmetic stays
within half of it over the whole value, clamp and layout batteries, and each planted defect -- applied inside the emulation on a
battery case where it can act -- is rejected by it.

What the comparison of tests/test_attn_gpu.py::test_fused_adamw_matches_torch_adamw_and_writes_the_shadows --
allclose(p, p_torch, rtol=2e-6, atol=2e-7), restated on p against the fp64 reference -- says of each defect ON THAT SAME CASE
(asserted below; |err| / bound of p' in brackets):
    accepts:  wd_after_update (7.3); shadow_truncated (p is untouched; the old test's torch.equal on the shadow would catch it)
    rejects:  no_eps (NaN at the exactly-zero gradients with fresh moments, 0 / 0), eps_under_root (1e5), eps_scaled (86),
              bc_from_t_minus_1 (71), bc2_without_root (5e4), wd_of_neighbour (84), m_from_unclamped_g, v_from_g, clamp_of_abs,
              tail_skipped, last_chunk_skipped, nan_to_minus_clip (NaN never compares close)
The old comparison rejects them HERE because these cases have what its own inputs never had: |g| from 1e-4 down to 4e-18, where
eps decides the update; exact zeros; |p| down to 0.01, where atol = 2e-7 no longer hides 1e-4 of an update of 3e-3; clipped
gradients next to unclipped ones; NaN.  On its own N(0, 1) inputs eps moves the update by 1e-8 of itself -- below fp32, so no
bound can see a missing eps there either; the batteries are what closes that gap, the bound what makes them pass or fail element
by element.  No old test compared m' or v' at all: m_from_unclamped_g and v_from_g exceed those bounds by 1e6.
"""
import pytest
import torch

import adamw_ref as R


def _step(L, r, defect=None, wd_neighbour=None):
    """(emulation outputs, reference) of one record of a launch"""
    args = (r["p"], r["g"], r["m"], r["v"], L["t"], r["lr"], r["wd"], L["betas"], L["eps"], L["clip"])
    return R.emulate(*args, defect=defect, wd_neighbour=wd_neighbour), R.reference(*args)


def _ratios(e, ref):
    out = {}
    for k in "pmv":
        out[k], msg = R.excess(e[k], ref[k], ref["tol_" + k])
        assert msg is None, (k, msg)
    return out


def _rejected(e, ref, kinds="pmv"):
    return any(R.excess(e[k], ref[k], ref["tol_" + k])[1] is not None for k in kinds)


LAUNCHES = R.value_launches() + [R.clamp_launch(1.0), R.clamp_launch(None), R.layout_launch()]


@pytest.mark.parametrize("L", LAUNCHES, ids=lambda L: "t%d-b%g-clip%s-%d" % (L["t"], L["betas"][0], L["clip"], len(L["records"])))
def test_emulation_stays_within_half_the_bound(L):
    """|err| / tol <= 0.5 for p', m' and v' of every record; every intermediate of the emulation is zero or a normal fp32 number
    (where the gradient is finite).  Largest ratios over all batteries: p' 0.37, m' 0.31, v' 0.29 -- the rounding terms, counted
    twice, against roundings that rarely all fall at their worst.  Per launch the largest ratio is 0.22 .. 0.37 for p', 0.15 ..
    0.31 for m' (0.15 with fresh moments, where one of the two products is exactly 0) and 0.23 .. 0.29 for v': the bound is
    nowhere looser than 1/20 at a launch's worst element.  The one term with more room than that is the powf term at t = 2
    and 3 (b2 = 0.999: 2 u b^t / (1 - b^t) = 998 u and 665 u on the bias correction, of which a correctly rounded powf can use half and
    at these two arguments uses 112 u and 105 u; 5.5 u of 199 u at t = 10); these ratios do not isolate it, because with |upd| of about lr |p| the roundings of q weigh as much in p'."""
    worst = dict.fromkeys("pmv", 0.0)
    for r in L["records"]:
        e, ref = _step(L, r)
        fin = torch.isfinite(r["g"])
        assert R.all_zero_or_normal([x[fin] for x in e["mids"]]), "an intermediate is subnormal or not finite"
        for k, x in _ratios(e, ref).items():
            worst[k] = max(worst[k], x)
        nan = torch.isnan(r["g"])
        assert all(bool(torch.isnan(e[k][nan]).all()) and bool(torch.isnan(ref[k][nan]).all()) for k in "pmv")
        assert bool(torch.isnan(e["shadow"][nan].float()).all())
    print("largest |err| / bound: " + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(x <= 0.5 for x in worst.values()), worst


def test_the_value_battery_holds_what_it_is_about():
    eps = R.f32(R.EPS)
    for L in R.value_launches():
        root = torch.cat([R.reference(r["p"], r["g"], r["m"], r["v"], L["t"], r["lr"], r["wd"], L["betas"], L["eps"])["root"]
                          for r in L["records"]])
        live = root > 0
        assert bool((root[live] < eps / 100).any()) and bool(((root > eps / 3) & (root < 3 * eps)).any()) and bool((root > 100 * eps).any())
        assert sorted({len(r["g"]) % 4 for r in L["records"]}) == [0, 3]          # vector and scalar path
        for r in L["records"]:
            g = r["g"]
            assert bool((g == 0).any()) and float(g.abs()[g != 0].min()) >= 4e-18
            if L["t"] > 1:
                m1 = R.reference(r["p"], g, r["m"], r["v"], L["t"], r["lr"], r["wd"], L["betas"], L["eps"])
                S = m1["tol_m"] / (6 * R.U)
                assert bool(((m1["m"].abs() < 1e-6 * S) & (S > 0)).any())        # m' cancels
                assert bool((r["m"] > 0).any()) and bool((r["m"] < 0).any())
                assert bool(((g == 0) & (r["m"] == 0) & (r["v"] == 0)).any())
            else:
                assert not bool(r["m"].any()) and not bool(r["v"].any())
    assert [L["t"] for L in R.value_launches()] == [1, 2, 3, 10, 1000, 100000, 3] and R.value_launches()[-1]["betas"] == (0.5, 0.9)


def test_the_clamp_battery_holds_what_it_is_about():
    one = torch.tensor(1.0)
    inside, outside = torch.nextafter(one, torch.tensor(0.0)), torch.nextafter(one, torch.tensor(2.0))
    for clip in (1.0, None):
        L = R.clamp_launch(clip)
        lanes = {k: set() for k in ("nan", "inf", "edge")}
        for r in L["records"]:
            g = r["g"]
            for s in (1.0, -1.0):
                assert all(bool((g == s * x).any()) for x in (one, inside, outside)) or len(g) < 16
            bits = g.view(torch.int32)
            assert bool((torch.isnan(g) & (bits < 0)).any()) and bool((torch.isnan(g) & (bits > 0)).any())       # -NaN and NaN
            assert bool((g == float("inf")).any()) and (len(g) < 16 or bool((g == float("-inf")).any()))
            if len(g) % 4 == 0:
                lanes["nan"] |= {int(i) % 4 for i in torch.isnan(g).nonzero()}
                lanes["inf"] |= {int(i) % 4 for i in torch.isinf(g).nonzero()}
                edges = (g.abs() == one) | (g.abs() == inside) | (g.abs() == outside)
                lanes["edge"] |= {int(i) % 4 for i in edges.nonzero()}
        assert lanes["nan"] == {0, 1, 2, 3} and lanes["inf"] == {0, 1, 2, 3} and lanes["edge"] == {0, 1, 2, 3}
    # the reference is torch.clamp and then the step: NaN stays, +-inf becomes +-clip
    g = torch.tensor([float("nan"), float("inf"), float("-inf"), 2.0])
    z = torch.zeros(4)
    ref = R.reference(torch.ones(4), g, z, z, 1, 1e-2, 0.0, clip=1.0)
    assert bool(torch.isnan(ref["m"][0])) and ref["m"][1:].tolist() == pytest.approx([0.1, -0.1, 0.1], rel=1e-6)
    ref = R.reference(torch.ones(4), g, z, z, 1, 1e-2, 0.0, clip=None)
    assert bool(torch.isnan(ref["p"][:3]).all()) and ref["m"][1:3].tolist() == [float("inf"), float("-inf")] and bool(torch.isnan(ref["m"][0]))


def test_the_layout_battery_holds_what_it_is_about():
    L = R.layout_launch()
    recs = L["records"]
    at, size = R.place(recs)
    assert L["t"] > 5 and sorted({r["n"] for r in recs}) == sorted(R.LENGTHS)
    for n in R.OFFSET_LENGTHS:
        assert n % 4 == 0
        offs = sorted((k, o) for r in recs if r["n"] == n for k, o in r["off"].items() if o)
        assert offs == sorted((k, o) for k in "pgmvs" for o in (1, 2, 3))
    assert all(sum(1 for o in r["off"].values() if o) <= 1 for r in recs)
    assert any(not r["shadow"] for r in recs) and {(r["lr"], r["wd"]) for r in recs} == set(R.LR_WD)
    assert any(r["wd"] == 0 for r in recs) and any(r["lr"] == 0 for r in recs)
    for k in "pgmvs":                       # no two tensors closer than GAP; the arena starts and ends with GAP canaries
        spans = sorted((a[k], a[k] + r["n"]) for a, r in zip(at, recs) if a[k] is not None)
        assert spans[0][0] >= R.GAP and size[k] - spans[-1][1] >= R.GAP
        assert all(b[0] - a[1] >= R.GAP for a, b in zip(spans, spans[1:]))
        assert all((a[k] - r["off"][k]) % 4 == 0 for a, r in zip(at, recs) if a[k] is not None)
    ch = R.chunk_list(recs)
    assert len(ch) == sum((r["n"] + R.CHUNK - 1) // R.CHUNK for r in recs) > 100
    sh = R.chunk_list(recs, shuffled=True)
    assert sorted(map(tuple, sh.tolist())) == sorted(map(tuple, ch.tolist())) and sh.tolist() != ch.tolist()
    total = sum(size.values()) + len(R.SWEEP_HIGH) * 65536 * 5 + sum(r["n"] * 5 for V in R.value_launches() for r in V["records"])
    assert total < 5 * 1.1e6                # "under about 1 M elements" per stream


def test_torchs_bf16_cast_is_round_to_nearest_even_on_the_whole_sweep():
    for high in R.SWEEP_HIGH:
        x = R.sweep_values(high)
        assert x.numel() == 65536 and bool(torch.isfinite(x).all()) and float(x.abs().min()) >= R.TINY
        assert torch.equal(R.bf16_bits(x.to(torch.bfloat16)), R.bf16_bits_rne(x))
    tie = R.sweep_values(0x3F80)[0x8000:0x8001], R.sweep_values(0x3F81)[0x8000:0x8001]
    assert int(R.bf16_bits(tie[0].to(torch.bfloat16))) == 0x3F80 and int(R.bf16_bits(tie[1].to(torch.bfloat16))) == 0x3F82
    assert int(R.bf16_bits(R.sweep_values(0x7F7F)[0x8000:0x8001].to(torch.bfloat16))) == 0x7F80     # rounds up to infinity


def test_excess_fails_nan_and_holds_nan_and_infinity_where_the_reference_has_them():
    ref = torch.tensor([1.0, float("nan"), float("inf"), 0.0], dtype=torch.float64)
    tol = torch.tensor([1e-6, float("nan"), float("nan"), 0.0], dtype=torch.float64)
    good = torch.tensor([1.0 + 5e-7, float("nan"), float("inf"), 0.0], dtype=torch.float64)
    assert R.excess(good, ref, tol) == (pytest.approx(0.5, rel=1e-3), None)
    for i, x in ((0, float("nan")), (0, 1.00001), (1, 1.0), (1, float("inf")), (2, float("-inf")), (2, float("nan")), (2, 3e38), (3, 1e-40)):
        bad = good.clone()
        bad[i] = x
        assert R.excess(bad, ref, tol)[1] is not None, (i, x)


# ---- planted defects ------------------------------------------------------------------------------------------------------------
def _value_record(t, scale, n):
    L = R.value_launch(t)
    return L, next(r for r in L["records"] if r["scale"] == scale and r["n"] == n)


def _clipped_case():
    """|g| in [0.4, 2.5] clipped at 1: elements inside and outside the clip"""
    L, r = _value_record(10, 1.0, 1024)
    return dict(L, clip=1.0), r


def _long_case():
    L = R.value_launch(10)
    return L, R.record(R.CHUNK + 8, 1.0, 10, key="long")


DEFECT_CASES = {   # defect: (case, the outputs the bound rejects it on, does the old allclose on p accept it on that case)
    "no_eps": (lambda: _value_record(1000, 1e-4, 1024), "p", False),
    "eps_under_root": (lambda: _value_record(1000, 1e-4, 1024), "p", False),
    "eps_scaled": (lambda: _value_record(2, 1e-4, 1024), "p", False),
    "bc_from_t_minus_1": (lambda: _value_record(1000, 1.0, 1024), "p", False),
    "bc2_without_root": (lambda: _value_record(1000, 1.0, 1024), "p", False),
    "wd_after_update": (lambda: _value_record(1000, 1.0, 1024), "p", True),
    "wd_of_neighbour": (lambda: _value_record(1000, 1.0, 1024), "p", False),
    "m_from_unclamped_g": (_clipped_case, "pm", False),
    "v_from_g": (lambda: _value_record(10, 1.0, 1024), "pv", False),
    "clamp_of_abs": (_clipped_case, "pm", False),
    "nan_to_minus_clip": (lambda: (R.clamp_launch(1.0), R.clamp_launch(1.0)["records"][0]), "pmv", False),
    "tail_skipped": (lambda: _value_record(10, 1.0, 1027), "pmv", False),
    "last_chunk_skipped": (_long_case, "pmv", False),
}


def test_every_defect_has_a_case():
    assert set(DEFECT_CASES) | {"shadow_truncated"} == set(R.DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECT_CASES))
def test_planted_defect_is_rejected_where_it_can_act(defect):
    case, kinds, old_accepts = DEFECT_CASES[defect]
    L, r = case()
    clean, ref = _step(L, r)
    assert not _rejected(clean, ref) and R.old_allclose_accepts(clean["p"][torch.isfinite(ref["p"])], ref["p"][torch.isfinite(ref["p"])])
    e, _ = _step(L, r, defect, wd_neighbour=0.0)       # the neighbouring record's wd: another group's 0
    for k in kinds:
        ratio, msg = R.excess(e[k], ref[k], ref["tol_" + k])
        print("%s %s': |err| / bound %.3g" % (defect, k, ratio))
        assert msg is not None, (defect, k)
    for k in set("pmv") - set(kinds):
        assert not _rejected(e, ref, k), (defect, k)    # ... and on nothing it does not touch
    got = R.old_allclose_accepts(e["p"], ref["p"])
    print("%s: the old allclose on p %s it" % (defect, "accepts" if got else "rejects"))
    assert got == old_accepts


def test_nan_gradient_turned_into_minus_clip_without_clipping_too():
    """clip = inf: the NaN becomes -inf, m' = -inf, v' = +inf, p' = NaN -- p' agrees with the reference by accident, m' and v' do not"""
    L = R.clamp_launch(None)
    r = L["records"][0]
    e, ref = _step(L, r, "nan_to_minus_clip")
    nan = torch.isnan(r["g"])
    assert bool(torch.isinf(e["m"][nan]).all()) and bool(torch.isinf(e["v"][nan]).all())
    assert _rejected(e, ref, "m") and _rejected(e, ref, "v") and not _rejected(e, ref, "p")


def test_truncated_shadow_differs_from_the_rounded_one():
    L, r = _value_record(10, 1.0, 1024)
    clean, ref = _step(L, r)
    e, _ = _step(L, r, "shadow_truncated")
    assert torch.equal(R.bf16_bits(clean["shadow"]), R.bf16_bits_rne(clean["p"]))
    assert not torch.equal(R.bf16_bits(e["shadow"]), R.bf16_bits(clean["shadow"]))
    assert torch.equal(e["p"], clean["p"]) and R.old_allclose_accepts(e["p"], ref["p"])
