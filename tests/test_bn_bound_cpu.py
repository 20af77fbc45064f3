"""The per-element bound of tests/bn_ref.py, checked without a GPU: an fp32 emulation of the kernels' arithmetic (chunk, phase
and fold order, the pivot) stays inside it, the defects the whole-tensor norms of test_fused_batchnorm_relu_maxpool_point_major
accept are rejected by it, its fp32 part stays well below its bf16 part, the undecided and contested caps hold for every input
of tests/test_bn_bound_gpu.py, and depth() counts the partials as bq_bn_chunks does."""
import pytest
import torch

import bn_ref as B

R_DEF, C_DEF, S_DEF = 16 * 529, 64, 16        # the planted defects: 34 partials, the last of 16 rows / one group
EPS, MOM = 1e-5, 0.1


def _ratio(out, ref, tol):
    r, msg = B.excess(out, ref, tol)
    assert msg is None, msg
    return r


def _rejected(out, ref, tol):
    return B.excess(out, ref, tol)[1] is not None


def _bf(t):
    return t.to(torch.bfloat16)


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
EMU_SHAPES = [(1, 8, 0), (3, 8, 0), (300, 8, 0), (300, 256, 0), (300, 2048, 0), (257, 512, 0), (1500, 64, 0), (8453, 8, 0),
              (33041, 8, 0), (37, 8, 1), (510, 64, 2), (80, 8, 16), (528, 8, 16), (8464, 64, 16), (64, 8, 64), (320, 8, 64),
              (576, 256, 64), (768, 256, 256), (576, 2048, 64), (1536, 512, 512), (16384, 8, 8192)]


@pytest.mark.parametrize("R,C,S", EMU_SHAPES, ids=lambda v: str(v))
def test_emulation_stays_within_the_bound(R, C, S):
    """emulate_stats / emulate_apply / emulate_backward (fp32; per-thread serial sums, the rps phase adds, fold_column or
    bn_fold_kernel with their 8 accumulators and tails; torch.rsqrt; one bf16 rounding) against the fp64 reference, ReLU on
    and off, pooled where S > 0, the table-reading reduce where it exists.  (33041, 8) has 130 partials.  Largest |err| / bound
    reached over the shapes:
        mean 0.473  rstd 0.233  scale 0.355  shift 0.287  running_mean 0.409  running_var 0.358
        y 0.996  y_pool 0.996  dx 0.996  dgamma 0.19  dbeta 0.0217  dgamma_arg 0.159  dbeta_arg 0.0118
    -- the bf16 outputs sit just below 1 because round-to-nearest reaches 2^-8 relative just above a power of two; the fp32
    outputs show how far the depth bound is from the rounding errors of this particular (random) data."""
    d = B.inputs(R, C, S)
    x, pool = d["x"], S > 0
    worst = {}
    f = B.stats(x, d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"])
    es, erm, erv = B.emulate_stats(x, d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"])
    for k, v in (("scale", es[0]), ("shift", es[1]), ("mean", es[2]), ("rstd", es[3]), ("running_mean", erm), ("running_var", erv)):
        worst[k] = _ratio(v, f[k], f["tol_" + k])
    st = B.given_stats(x, d["gamma"], d["beta"], EPS)
    for relu in (True, False):
        a = B.apply(x, st[0], st[1], S, relu, pool)
        ey, earg = B.emulate_apply(x, st[0], st[1], S, relu, pool)
        k = "y_pool" if pool else "y"
        worst[k] = max(worst.get(k, 0.0), _ratio(ey, a["y"], a["tol_y"]))
        b = B.backward(d["dy"], x, st, S, relu, pool)
        if pool:
            assert torch.equal(earg, b["arg"])
        outs = dict(zip(("dx", "dgamma", "dbeta"), B.emulate_backward(d["dy"], x, st, S, relu, pool)))
        for k, v in outs.items():
            worst[k] = max(worst.get(k, 0.0), _ratio(v, b[k], b["tol_" + k]))
        if "tol_dbeta_arg" in b:
            _, tg, tb = B.emulate_backward(d["dy"], x, st, S, relu, pool, table=b["arg"])
            worst["dgamma_arg"] = max(worst.get("dgamma_arg", 0.0), _ratio(tg, b["dgamma"], b["tol_dgamma_arg"]))
            worst["dbeta_arg"] = max(worst.get("dbeta_arg", 0.0), _ratio(tb, b["dbeta"], b["tol_dbeta_arg"]))
    print("(%d, %d, %d) largest |err| / bound: %s" % (R, C, S, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("R,C,S", [(300, 64, 0), (8464, 64, 16), (1500, 256, 0)])
def test_fp32_part_of_the_bound_stays_below_the_bf16_part(R, C, S, relu):
    """in EVERY ordinary channel (8 and up) the fp32 error e is at most a tenth of the bf16 rounding 2^-8 |r| (in the mean over
    the channel: single elements near a zero of r have no bf16 part to compare with)"""
    d = B.inputs(R, C, S)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    a = B.apply(d["x"], st[0], st[1], S, relu, S > 0)
    b = B.backward(d["dy"], d["x"], st, S, relu, S > 0)
    for name, e, r in (("y", a["e_y"], a["y"]), ("dx", b["e_dx"], b["dx"])):
        share = e[:, 8:].mean(0) / (B.B8 * r[:, 8:].abs().mean(0))
        assert float(share.max()) <= 0.1, "%s: fp32 part / bf16 part = %.3g in channel %d" % (
            name, float(share.max()), 8 + int(share.argmax()))


# ---- planted defects ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """the fp64 results at (8464, 64): pooled over 16 and unpooled, both with ReLU and without sentinels; statistics of the
    pooled input"""
    out = {}
    for key, S in (("p", S_DEF), ("u", 0)):
        d = B.inputs(R_DEF, C_DEF, S, "plain")
        st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
        out[key] = dict(d=d, st=st, a=B.apply(d["x"], st[0], st[1], S, True, S > 0), b=B.backward(d["dy"], d["x"], st, S, True, S > 0))
    d = out["p"]["d"]
    out["f"] = B.stats(d["x"], d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"])
    return out


def _dx_with(p, g=None, mb=None):
    """the pooled dx of the reference with another routed gradient g or another dbeta / R"""
    sc, _, mu, rs = (p["st"][i].double() for i in range(4))
    b = p["b"]
    xhat = (p["d"]["x"].double() - mu) * rs
    return sc * ((b["g"] if g is None else g) - (b["dbeta"] / R_DEF if mb is None else mb) - xhat * b["dgamma"] / R_DEF)


def _route(p, arg):
    d, b = p["d"], p["b"]
    G = R_DEF // S_DEF
    zsel = b["g"].view(G, S_DEF, C_DEF).gather(1, b["arg"][:, None])[:, 0]       # the reference's routed (masked) gradient
    return torch.zeros(G, S_DEF, C_DEF, dtype=torch.float64).scatter_(1, arg[:, None], zsel[:, None]).view(R_DEF, C_DEF)


def test_the_clean_results_pass_norms_and_bound(planted):
    for key in ("p", "u"):
        a, b = planted[key]["a"], planted[key]["b"]
        assert B.old_norms_accept("y", _bf(a["y"]), a["y"]) and not _rejected(_bf(a["y"]), a["y"], a["tol_y"])
        assert B.old_norms_accept("dx", _bf(b["dx"]), b["dx"]) and not _rejected(_bf(b["dx"]), b["dx"], b["tol_dx"])
    assert torch.allclose(_dx_with(planted["p"]), planted["p"]["b"]["dx"], rtol=1e-12, atol=1e-14)
    assert torch.equal(_route(planted["p"], planted["p"]["b"]["arg"]), planted["p"]["b"]["g"])


def _stats_without(x, rows):
    """mean and var as the kernels form them, the rows' terms missing from both sums (still divided by R)"""
    xd = x.double()
    t = xd - xd[0]
    keep = torch.ones(x.shape[0], 1, dtype=torch.float64)
    keep[rows] = 0.0
    dm, q = (t * keep).mean(0), (t.square() * keep).mean(0)
    return xd[0] + dm, (q - dm * dm).clamp_min(0.0)


def _y_from(x, gamma, beta, mean, var):
    """the pooled ReLU output under other statistics"""
    scale = gamma.double() * (var + B._f32(EPS)).rsqrt()
    z = x.double() * scale + (beta.double() - mean * scale)
    return z.view(R_DEF // S_DEF, S_DEF, C_DEF).amax(1).clamp_min(0.0)


@pytest.mark.parametrize("rows", [slice(R_DEF - 1, R_DEF), slice(33 * 256, R_DEF)], ids=["last-row", "partial-33"])
def test_defect_statistics_lose_the_last_row_or_the_tail_partial(planted, rows):
    """the last row of the ragged chunk never added; partial 33, which fold_column's tail loop adds (phase 1: 1, 5 .. 29 in the
    unrolled trip, then 33), never added.  The output y under those statistics passes the old 6e-3 (rel-L2 1.6e-3 and 2.5e-3).
    The old 1e-4 on the running statistics does NOT accept either at this shape (running_mean 4.9e-4 / 7.3e-3, running_var
    1.3e-3 / 1.9e-2; on the ordinary channels alone 1.6e-4 / 2.4e-3 and 2.1e-4 / 3.2e-3): one row of 8464 is 1.2e-4 of the
    sums.  Kept: the bound rejects mean, rstd, running_mean and running_var by one to three orders of magnitude."""
    d, f = planted["p"]["d"], planted["f"]
    mean, var = _stats_without(d["x"], rows)
    m = B._f32(MOM)
    rmean = (1.0 - m) * d["rm"].double() + m * mean
    rvar = (1.0 - m) * d["rv"].double() + m * var * (R_DEF / (R_DEF - 1.0))
    y_ref = _y_from(d["x"], d["gamma"], d["beta"], f["mean"], f["var"])
    assert B.old_norms_accept("y", _bf(_y_from(d["x"], d["gamma"], d["beta"], mean, var)), y_ref)
    assert not B.old_norms_accept("running_mean", rmean, f["running_mean"])
    assert not B.old_norms_accept("running_var", rvar, f["running_var"])
    assert _rejected(mean.float(), f["mean"], f["tol_mean"])
    assert _rejected((var + B._f32(EPS)).rsqrt().float(), f["rstd"], f["tol_rstd"])
    assert _rejected(rmean.float(), f["running_mean"], f["tol_running_mean"])
    assert _rejected(rvar.float(), f["running_var"], f["tol_running_var"])


def test_defect_backward_sums_lose_the_last_group_of_one_lane(planted):
    """the ragged partial's only group never added by the thread of channels 24 .. 31: dgamma passes the old 1e-2 (rel-L2
    9.2e-3), dbeta just does not (1.16e-2; one of the eight channels alone: 2.4e-3); the bound rejects both"""
    b, cols = planted["p"]["b"], slice(24, 32)
    last = b["g"][R_DEF - S_DEF:]
    sc, _, mu, rs = (planted["p"]["st"][i].double() for i in range(4))
    xhat = (planted["p"]["d"]["x"][R_DEF - S_DEF:].double() - mu) * rs
    db, dg = b["dbeta"].clone(), b["dgamma"].clone()
    db[cols] -= last.sum(0)[cols]
    dg[cols] -= (last * xhat).sum(0)[cols]
    assert float(last.abs().sum(0)[cols].min()) > 0
    assert B.old_norms_accept("dgamma", dg, b["dgamma"]) and not B.old_norms_accept("dbeta", db, b["dbeta"])
    one = b["dbeta"].clone()
    one[24] = db[24]
    assert B.old_norms_accept("dbeta", one, b["dbeta"]) and _rejected(one.float(), b["dbeta"], b["tol_dbeta"])
    for sfx in ("", "_arg"):
        assert _rejected(db.float(), b["dbeta"], b["tol_dbeta" + sfx]) and _rejected(dg.float(), b["dgamma"], b["tol_dgamma" + sfx])


def test_defect_a_partial_of_the_fold_tail_missing_from_dbeta(planted):
    """partial 32 (bn_fold_kernel: phase 0 adds 0, 16, 32, all in its tail loop) never added: 16 of 529 groups.  The old norms
    do NOT accept this one at this shape (rel-L2 0.17 against 1e-2) -- kept, as the bound must reject it whatever the norms do"""
    b = planted["p"]["b"]
    rows = slice(32 * 256, 33 * 256)
    db = b["dbeta"] - b["g"][rows].sum(0)
    assert not B.old_norms_accept("dbeta", db, b["dbeta"])
    assert _rejected(db.float(), b["dbeta"], b["tol_dbeta"]) and _rejected(db.float(), b["dbeta"], b["tol_dbeta_arg"])


def test_defect_last_maximum_instead_of_first(planted):
    """`>=` in the search: the gradient of a tied group goes to the last copy, the arg byte names it; y does not change.  The old
    dx norm does NOT accept this here (rel-L2 1.41; 0.55 on the ordinary channels): a fifth of the (group, channel) pairs are
    planted ties and the constant channel is one tie throughout -- on the old test's random inputs only the natural ties move
    (169 of the 29624 untied ordinary pairs here).  Kept: every moved gradient leaves the bound, every moved byte the table"""
    p = planted["p"]
    d, b = p["d"], p["b"]
    G = R_DEF // S_DEF
    z = B._z(d["x"], p["st"][0], p["st"][1])[0].view(G, S_DEF, C_DEF)
    last = torch.where(z == z.amax(1, keepdim=True), torch.arange(S_DEF).view(1, S_DEF, 1), -1).amax(1)
    moved = last != b["arg"]
    assert bool(moved[d["tied"]].all()) and int(moved.sum()) >= int(d["tied"].sum())
    assert not torch.equal(last.to(torch.uint8), p["a"]["arg"])
    dx = _dx_with(p, g=_route(p, last))
    assert not B.old_norms_accept("dx", _bf(dx), b["dx"])
    err = (_bf(dx).double() - b["dx"]).abs().view(G, S_DEF, C_DEF)
    off = (err > b["tol_dx"].view(G, S_DEF, C_DEF)).any(1)
    live = b["g"].view(G, S_DEF, C_DEF).abs().sum(1) * p["st"][0].double().abs() > 0
    assert torch.equal(off, moved & live)


def test_defect_relu_mask_not_strict(planted):
    """`>=` for `>`: the elements with z == 0 exactly (channels 4 and 7: the 16 planted ones and the rows that drew the value v
    by themselves) let their dy through; they are decided, tolerance as for any other element, and dbeta of the two channels
    moves by whole dy values.  The old dx norm accepts it; the old dbeta norm does not quite (rel-L2 1.5e-2 against 1e-2: the
    two channels hold 36 such elements)"""
    p = planted["u"]
    d, b = p["d"], p["b"]
    z = B._z(d["x"], p["st"][0], p["st"][1])[0]
    zero = z == 0
    assert int(zero.sum()) >= 16 and not bool(zero[:, [c for c in range(C_DEF) if c not in B.EXACT]].any()) and b["undecided"] == 0
    g = b["g"] + d["dy"].double() * zero
    sc, _, mu, rs = (p["st"][i].double() for i in range(4))
    xhat = (d["x"].double() - mu) * rs
    db, dg = g.sum(0), (g * xhat).sum(0)
    dx = sc * (g - db / R_DEF - xhat * dg / R_DEF)
    assert B.old_norms_accept("dx", _bf(dx), b["dx"]) and not B.old_norms_accept("dbeta", db, b["dbeta"])
    assert _rejected(_bf(dx), b["dx"], b["tol_dx"])
    assert _rejected(db.float(), b["dbeta"], b["tol_dbeta"])


def test_defect_pooled_dx_divides_dbeta_by_the_group_count(planted):
    """dbeta / (R / S) for dbeta / R.  The old dx norm does NOT accept it at this shape (rel-L2 0.3 against 2e-2: the term is
    15 dbeta / R on every row, and only R >~ 5e5 rows make it small against the routed gradients) -- kept"""
    p = planted["p"]
    b = p["b"]
    dx = _dx_with(p, mb=b["dbeta"] / (R_DEF // S_DEF))
    assert not B.old_norms_accept("dx", _bf(dx), b["dx"])
    assert _rejected(_bf(dx), b["dx"], b["tol_dx"])


def test_defect_two_channels_swapped_inside_a_lanes_eight(planted):
    """channels 26 and 29 of one pooled output row and of one dx row change places"""
    p = planted["p"]
    a, b = p["a"], p["b"]
    y, dx = a["y"].clone(), b["dx"].clone()
    y[100, [26, 29]] = a["y"][100, [29, 26]]
    dx[4001, [26, 29]] = b["dx"][4001, [29, 26]]
    assert B.old_norms_accept("y", _bf(y), a["y"]) and B.old_norms_accept("dx", _bf(dx), b["dx"])
    assert _rejected(_bf(y), a["y"], a["tol_y"]) and _rejected(_bf(dx), b["dx"], b["tol_dx"])


def test_defect_one_wrong_arg_byte(planted):
    """one byte of the table one row off: the routed gradient lands on the neighbour row (dx), and the table-reading reduce
    forms dgamma with that row's xhat"""
    p = planted["p"]
    d, b = p["d"], p["b"]
    gi, c = 200, 9
    arg = b["arg"].clone()
    arg[gi, c] = (arg[gi, c] + 1) % S_DEF
    assert not torch.equal(arg.to(torch.uint8), p["a"]["arg"])
    g = _route(p, arg)
    dx = _dx_with(p, g=g)
    sc, _, mu, rs = (p["st"][i].double() for i in range(4))
    dg = (g * (d["x"].double() - mu) * rs).sum(0)
    assert float(g.abs().sum(0)[c]) > 0 and float((g - b["g"]).abs().sum()) > 0
    assert B.old_norms_accept("dx", _bf(dx), b["dx"]) and B.old_norms_accept("dgamma", dg, b["dgamma"])
    assert _rejected(_bf(dx), b["dx"], b["tol_dx"])
    assert _rejected(dg.float(), b["dgamma"], b["tol_dgamma_arg"])


def test_defect_pivot_from_the_wrong_channel_group(planted):
    """the pivot of channel c read at column c + 8 (the next thread's group), in both kernels: mathematically the same mean and
    variance, but channel 1 (mean 40, std 0.5) now sums squares of ~1600 in fp32.  Emulated in fp32; the output under those
    statistics passes the old norm, rstd of channel 1 leaves the bound"""
    d, f = planted["p"]["d"], planted["f"]
    good, _, _ = B.emulate_stats(d["x"], d["gamma"], d["beta"], EPS, MOM)
    bad, _, _ = B.emulate_stats(d["x"], d["gamma"], d["beta"], EPS, MOM, pivot_roll=8)
    assert not _rejected(good[3], f["rstd"], f["tol_rstd"])
    y_ref = B.apply(d["x"], good[0], good[1], S_DEF, True, True)["y"]
    assert B.old_norms_accept("y", B.emulate_apply(d["x"], bad[0], bad[1], S_DEF, True, True)[0], y_ref)
    assert _rejected(bad[3], f["rstd"], f["tol_rstd"])
    err = (bad[3].double() - f["rstd"]).abs()
    assert float(err[B.CH_MEAN40]) > f["tol_rstd"][B.CH_MEAN40]


def test_defect_running_var_takes_the_biased_variance(planted):
    """the old 1e-4 accepts it on the ordinary channels (rel-L2 5.2e-5); over all 64 it reads 1.18e-4 = 1 / R, because channel 3
    (scaled by 24: running_var 414) is nearly all of that norm"""
    d, f = planted["p"]["d"], planted["f"]
    m = B._f32(MOM)
    rvar = (1.0 - m) * d["rv"].double() + m * f["var"]
    assert B.old_norms_accept("running_var", rvar[8:], f["running_var"][8:])
    assert _rejected(rvar.float(), f["running_var"], f["tol_running_var"])


# ---- caps and bookkeeping over the GPU module's cases -----------------------------------------------------------------------------
def _bq_bn_chunks(R, S, pool):
    """bq_bn_chunks of csrc/bn.hip, restated literally"""
    if R <= 0:
        return 0
    cr = 1024 if R >= (1 << 20) else 256
    if pool and S > 0:
        G = R // S
        gpc = cr // S if cr // S > 0 else 1
        return (G + gpc - 1) // gpc
    return (R + cr - 1) // cr


def test_depth_counts_the_partials_as_bq_bn_chunks():
    for c in B.STATS_CASES:
        assert B.depth(c["R"], c["C"])[1] == _bq_bn_chunks(c["R"], 0, 0)
    assert sorted({B.depth(c["R"], 8)[1] for c in B.STATS_CASES if c["C"] == 8 and c["R"] < 40000}) == [1, 2, 5, 17, 34, 130]
    for c in B.BWD_CASES + B.TABLE_CASES:
        D, n_c = B.depth(c["R"], c["C"], c["S"], c["pool"], backward=True)
        assert n_c == _bq_bn_chunks(c["R"], c["S"], c["pool"]) and 1 <= D <= (c["R"] // c["S"] if c["pool"] else c["R"])
    for c in B.TABLE_CASES:
        n, per, ph, n_c = B.layout(c["R"], c["C"], c["S"], True, True)
        assert n_c == _bq_bn_chunks(c["R"], c["S"], 1) and per == -(-n // n_c) and n_c * per >= n and ph == 256 // c["C"]
    assert B.depth(B.BIG_LO, 8)[1] == 4096 and B.depth(B.BIG_HI, 8)[1] == 1025
    assert B.depth(B.BIG_LO, 8, 64, True)[1] == 4096 and B.depth(B.BIG_HI, 8, 64, True)[1] == 1025
    assert B.depth(300, 2048)[0] == min(256 + 1 + 1, 300) and B.depth(1, 8)[0] == 1
    # the fold's own chain where it is longer than ceil(n_c / 4): bn_fold_kernel's 16 phase sums in order, fold_column's tail
    assert B.fold_depth(34, 16) == 2 + 15 and B.fold_depth(28, 4) == 6 + 2 and B.fold_depth(1, 4) == 0 == B.fold_depth(1, 16)
    assert B.depth(8453, 64, backward=True)[0] == 8 + 32 + 17 and B.depth(8453, 64)[0] == 8 + 32 + 9
    assert B.fold_depth(4096, 4) < 1024 and B.fold_depth(4096, 16) < 1024


def test_caps_hold_for_every_input_of_the_gpu_module():
    """no contested group (apply() / backward() assert it) and at most 1e-4 undecided ReLU masks (backward() asserts it; the
    random inputs have none at all), for the statistics given to the backward cases"""
    seen = set()
    for c in B.APPLY_CASES:
        d = B.inputs(c["R"], c["C"], c["S"])
        st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
        a = B.apply(d["x"], st[0], st[1], c["S"], c["relu"], c["pool"])
        assert (a["arg"] is not None) == c["pool"]
    for c in B.BWD_CASES + B.TABLE_CASES:
        key = (c["R"], c["C"], c["S"], c["relu"])
        if key in seen:
            continue
        seen.add(key)
        d = B.inputs(c["R"], c["C"], c["S"])
        st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
        b = B.backward(d["dy"], d["x"], st, c["S"], c["relu"], c["pool"])
        assert b["undecided"] == 0
        if c["pool"] and c["S"] >= 2:
            tied = d["tied"]
            assert int(tied.sum()) >= tied.numel() // 12 or tied.shape[0] < 50
            assert bool((b["arg"][tied] < c["S"] - 1).any())


def test_planted_ties_are_ties_and_some_have_a_negative_maximum():
    d = B.inputs(R_DEF, C_DEF, S_DEF)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    G = R_DEF // S_DEF
    z = B._z(d["x"], st[0], st[1])[0].view(G, S_DEF, C_DEF)
    zmax = z.amax(1)
    copies = (z == zmax[:, None]).sum(1)
    assert bool((copies[d["tied"]] >= 2).all()) and bool((copies[d["tied"]] >= 3).any())
    assert int((zmax[d["tied"]] < 0).sum()) > 100
    for ch in B.EXACT:                       # every seventh group of the exact channels: a tie at z == 0
        assert bool((zmax[3::7, ch] == 0).all()) and bool((copies[3::7, ch] >= 2).all())
    assert bool((zmax[:, B.CH_GAMMA0] == z[:, 0, B.CH_GAMMA0]).all()) and bool((copies[:, B.CH_GAMMA0] == S_DEF).all())
