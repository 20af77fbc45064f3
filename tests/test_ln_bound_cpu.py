"""The per-element bound of tests/ln_ref.py, checked without a GPU: an fp32 emulation of the kernels' arithmetic stays inside
it, the defects the whole-tensor norms of tests/test_attn_gpu.py accept are rejected by it, its fp32 part stays well below its
bf16 part, and the CPU restatement of the dropout / drop-path hashes keeps the share of elements it should."""
import math

import pytest
import torch

import ln_ref as R

M_DEF, H_DEF = 4101, 768          # the planted defects: five trips of the backward grid, a ragged second trip of the forward's
SEED = 777


def _ratio(out, ref, tol):
    r, msg = R.excess(out, ref, tol)
    assert msg is None, msg
    return r


@pytest.mark.parametrize("H", [256, 768, 1024])
def test_emulation_stays_within_the_bound(H):
    """The fp32 emulation (bf16 -> fp32, per-lane serial sums of 4 NCH terms then a 64-lane tree, torch.rsqrt, one bf16
    rounding; the backward's dgamma / dbeta in wave, workgroup and grid order) against the fp64 reference at M = 1541 with
    dropout, stochastic depth, a residual and dsum.  Largest |err| / bound reached over H = 256, 768, 1024:
        y 0.988  sum 0.996  mean 0.0037  rstd 0.0089  dx 0.995  dres 0.994  dgamma 0.001  dbeta 8.3e-05   (both backward forms)
    -- the bf16 outputs sit just below 1 because round-to-nearest reaches 2^-8 relative just above a power of two; the fp32
    outputs show how far the any-order summation bound is from this particular order."""
    M = 1541
    d = R.inputs(M, H)
    kscale, ps = R.masks(M, H, 0.1, 0.3, 7, SEED)
    worst = {}
    ref = R.forward(d["x"], d["res"], d["gamma"], d["beta"], 1e-6, kscale, ps)
    y, s, mean, rstd = R.emulate_forward(d["x"], d["res"], d["gamma"], d["beta"], 1e-6, kscale, ps)
    worst["y"] = _ratio(y, ref["y"], ref["tol_y"])
    worst["sum"] = _ratio(s, ref["z"], ref["tol_sum"])
    worst["mean"] = _ratio(mean, ref["mean"], ref["tol_mean"])
    worst["rstd"] = _ratio(rstd, ref["rstd"], ref["tol_rstd"])
    m32, r32 = R.stats32(ref["z"], 1e-6)
    for form in ("x", "sum"):
        if form == "x":
            args = (d["x"], d["res"], d["gamma"], d["dy"], d["dsum"], m32, r32, kscale, ps, False)
        else:
            sb = ref["z"].to(torch.bfloat16)
            ms, rs = R.stats32(sb.double(), 1e-6)
            args = (sb, None, d["gamma"], d["dy"], d["dsum"], ms, rs, None, ps, True)
        b = R.backward(*args)
        dx, dres, dg, db = R.emulate_backward(*args)
        for k, out, r, t in (("dx", dx, b["dx"], b["tol_dx"]), ("dres", dres, b["dz"], b["tol_dres"]),
                             ("dgamma", dg, b["dgamma"], b["tol_dgamma"]), ("dbeta", db, b["dbeta"], b["tol_dbeta"])):
            worst[k + "/" + form] = _ratio(out, r, t)
        assert bool((dx.float()[b["dropped"]] == 0).all())
    print("H=%d largest |err| / bound: %s" % (H, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), "emulation outside the bound at H=%d: %r" % (H, worst)


@pytest.mark.parametrize("H", [256, 1024])
def test_fp32_part_of_the_bound_stays_below_the_bf16_part(H):
    """On the ordinary random rows the fp32 error e is one to two orders of magnitude below the bf16 rounding 2^-8 |r| (in the
    mean over the tensor: single elements near a zero of r have no bf16 part to compare with)"""
    M = 64
    d = R.inputs(M, H)
    kscale, ps = R.masks(M, H, 0.1, 0.3, 7, SEED)
    rows = [r for r in range(M) if r not in R.SPECIAL_ROWS]
    ref = R.forward(d["x"], d["res"], d["gamma"], d["beta"], 1e-6, kscale, ps)
    m32, r32 = R.stats32(ref["z"], 1e-6)
    b = R.backward(d["x"], d["res"], d["gamma"], d["dy"], d["dsum"], m32, r32, kscale, ps)
    for name, e, r in (("y", ref["e_y"], ref["y"]), ("sum", ref["e_sum"], ref["z"]), ("dz", b["e_dz"], b["dz"])):
        share = float(e[rows].mean() / (R.B8 * r[rows].abs().mean()))
        assert share <= 0.1, "%s: fp32 part / bf16 part = %.3g at H=%d" % (name, share, H)


# ---- planted defects ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """the fp64 results at (4101, 768) with dropout 0.1, a residual and dsum; and the twin pair of two 4101-row groups' second"""
    M, H = M_DEF, H_DEF
    d = R.inputs(M, H)
    kscale, _ = R.masks(M, H, 0.1, 0.0, 0, SEED)
    f = R.forward(d["x"], d["res"], d["gamma"], d["beta"], 1e-12, kscale)
    m32, r32 = R.stats32(f["z"], 1e-12)
    b = R.backward(d["x"], d["res"], d["gamma"], d["dy"], d["dsum"], m32, r32, kscale)
    return dict(d=d, kscale=kscale, f=f, b=b, m32=m32, r32=r32)


def _bf(t):
    return t.to(torch.bfloat16)


def _rejected(out, ref, tol):
    return R.excess(out, ref, tol)[1] is not None


def test_the_clean_result_passes_norms_and_bound(planted):
    f, b = planted["f"], planted["b"]
    for out, ref, tol, grad in ((f["y"], f["y"], f["tol_y"], False), (b["dx"], b["dx"], b["tol_dx"], True),
                                (b["dz"], b["dz"], b["tol_dres"], True)):
        assert R.old_norms_accept(_bf(out), ref, grad) and not _rejected(_bf(out), ref, tol)


def test_defect_last_row_with_the_previous_strided_rows_statistics(planted):
    """row 4100 is the second trip of the wave that did row 4 (stride 4 x 1024): normalised with row 4's mean and rstd"""
    f, d = planted["f"], planted["d"]
    last, prev = M_DEF - 1, M_DEF - 1 - 4 * R.FWD_CAP
    y = f["y"].clone()
    y[last] = (f["z"][last] - f["mean"][prev]) * f["rstd"][prev] * d["gamma"].double() + d["beta"].double()
    assert R.old_norms_accept(_bf(y), f["y"])
    assert _rejected(_bf(y), f["y"], f["tol_y"])


def test_defect_one_lanes_columns_of_chunk_2_with_chunk_1s_gamma(planted):
    f, d = planted["f"], planted["d"]
    row, lane = 2049, 37
    c2, c1 = slice(512 + 4 * lane, 516 + 4 * lane), slice(256 + 4 * lane, 260 + 4 * lane)
    y = f["y"].clone()
    y[row, c2] = f["zhat"][row, c2] * d["gamma"].double()[c1] + d["beta"].double()[c2]
    assert R.old_norms_accept(_bf(y), f["y"])
    assert _rejected(_bf(y), f["y"], f["tol_y"])


def test_defect_backward_keep_mask_shifted_by_one_column(planted):
    """dx of one chunk of one row masked with the keep bits of the columns one to the right"""
    b, kscale = planted["b"], planted["kscale"]
    row = 3000
    dx = b["dx"].clone()
    dx[row, 256:512] = b["dz"][row, 256:512] * kscale[row, 257:513]
    assert not torch.equal(kscale[row, 256:512], kscale[row, 257:513])
    assert R.old_norms_accept(_bf(dx), b["dx"], grad=True)
    assert _rejected(_bf(dx), b["dx"], b["tol_dx"])


def test_defect_dsum_missing_from_dres_in_one_row(planted):
    b, d = planted["b"], planted["d"]
    row = 1537
    dres = b["dz"].clone()
    dres[row] -= d["dsum"][row].double()
    assert R.old_norms_accept(_bf(dres), b["dz"], grad=True)
    assert _rejected(_bf(dres), b["dz"], b["tol_dres"])


def test_defect_second_row_group_with_the_first_groups_gamma_on_4_columns(planted):
    """a twin launch of 2 x 4101 rows: group 1 (the same inputs, gamma2 / beta2) forms gd with gamma instead of gamma2 in one
    lane's 4 columns -- the lane where the two differ least among those that differ by at least 0.1 (25 bf16 steps) in all
    four, so that the defect is as quiet as a wrong-parameter defect gets"""
    d, kscale, m32, r32 = planted["d"], planted["kscale"], planted["m32"], planted["r32"]
    diff = (d["gamma2"] - d["gamma"]).abs().view(-1, 4)
    ok = diff.amin(1) >= 0.1
    lane = int(torch.where(ok, diff.amax(1), torch.full_like(diff[:, 0], math.inf)).argmin())
    cols = slice(4 * lane, 4 * lane + 4)
    g_bad = d["gamma2"].clone()
    g_bad[cols] = d["gamma"][cols]
    want = R.backward(d["x"], d["res"], d["gamma2"], d["dy"], None, m32, r32, kscale)
    got = R.backward(d["x"], d["res"], g_bad, d["dy"], None, m32, r32, kscale)
    # group 0 of the launch is right; the old norm ran over both groups
    both = lambda t1: torch.cat([planted["b"]["dx"], t1])
    assert R.old_norms_accept(_bf(both(got["dx"])), both(want["dx"]), grad=True)
    assert _rejected(_bf(got["dx"]), want["dx"], want["tol_dx"])
    assert _rejected(_bf(got["dz"]), want["dz"], want["tol_dres"])


def test_defect_one_workgroups_partial_missing_from_dgamma(planted):
    """workgroup 100 of the 384 (rows 400..403 of every trip) never adds its partial: fp32 output, the bound alone"""
    b, d, m32, r32, kscale = planted["b"], planted["d"], planted["m32"], planted["r32"], planted["kscale"]
    rows = torch.arange(M_DEF)
    mine = (rows % (4 * R.BWD_CAP)) // 4 == 100
    part = R.backward(d["x"][mine], d["res"][mine], d["gamma"], d["dy"][mine], d["dsum"][mine], m32[mine], r32[mine], kscale[mine])
    assert not _rejected((b["dgamma"]).float(), b["dgamma"], b["tol_dgamma"])
    assert _rejected((b["dgamma"] - part["dgamma"]).float(), b["dgamma"], b["tol_dgamma"])
    assert _rejected((b["dbeta"] - part["dbeta"]).float(), b["dbeta"], b["tol_dbeta"])


# ---- mask statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_keeps_its_share(p):
    n = 1 << 20
    keep = R.keep_mask(R.eff_seed(SEED, 12345), n // 1024, 1024, p)
    share = float(keep.double().mean())
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), share


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_path_mask_keeps_its_share_per_sample(p):
    n, rps = 1 << 20, 7
    keep = R.path_keep(R.eff_seed(SEED), n * rps, p, rps).view(n, rps)
    assert bool((keep == keep[:, :1]).all())            # a sample's rows share one draw
    share = float(keep[:, 0].double().mean())
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), share


def test_seed_mix_and_scales_are_the_launchers():
    assert R.eff_seed(5) == 5 and R.eff_seed(-1) == 0xFFFFFFFF
    assert R.eff_seed(7, 3) == (3 * 2654435761 + 7) % 2 ** 32
    assert R.eff_seed(7, -2) == ((2 ** 32 - 2) * 2654435761 + 7) % 2 ** 32      # the int32 seed tensor is read as unsigned
    assert R.thresh(0.5) == 2 ** 31 and R.thresh(0.0) == 0
    assert R.thresh(0.1) == int(float(torch.tensor(0.1)) * 2 ** 32) != int(0.1 * 2 ** 32)   # p is a C float on the way in
    assert R.inv_keep(0.5) == 2.0 and R.inv_keep(0.1) == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1)))
