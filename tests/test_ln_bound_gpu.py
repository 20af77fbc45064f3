"""The row kernels of csrc/ln.hip and csrc/ln_bwd_kernel_body.h (drop_add_ln_fwd / _bwd / _bwd_sum, the twin forms, the
deterministic backward) and gelu_fwd held to the per-element fp64 bounds of tests/ln_ref.py: one wrong row, lane, mask bit or
parameter group fails, where the whole-tensor norms of tests/test_attn_gpu.py accept it.  Every case calls the _ext wrappers
directly, moves the results to the CPU and compares every element; `not (err <= tol)` fails, so NaN fails.

The backward cases take mean and rstd computed in fp64 and rounded once to fp32 (and a test-made bf16 sum), so that a forward
defect cannot hide a backward one; test_backward_chained_to_the_kernels_own_forward feeds the kernel's own outputs instead.

The largest |err| / bound per output kind is printed at the end of the module (pytest -s).
"""
import pytest
import torch

import ln_ref as R

pytestmark = pytest.mark.gpu

SEED = 777
SEED_VALUE = -5          # the content of the int32 seed tensor: read as unsigned by ln_seed
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest |err| / bound per output kind: " + "  ".join("%s %.3g" % kv for kv in _WORST.items()))


@pytest.fixture(scope="module")
def ext(dev):
    from bridgeqa_amd import _ext
    return _ext


class _Hold:
    """collects the failures of one case; assert_ok() reports them all"""

    def __init__(self, name):
        self.name, self.fails = name, []

    def __call__(self, kind, out, ref, tol, what=None):
        ratio, msg = R.excess(out, ref, tol)
        _WORST[kind] = max(_WORST.get(kind, 0.0), ratio)
        if msg:
            self.fails.append("%s %s: %s" % (self.name, what or kind, msg))

    def true(self, cond, msg):
        if not cond:
            self.fails.append("%s: %s" % (self.name, msg))

    def assert_ok(self):
        assert not self.fails, "\n".join(self.fails)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items())


def _seed_args(dev, st):
    """(seed tensor or None, its value or None)"""
    return (torch.tensor([SEED_VALUE], dtype=torch.int32, device=dev), SEED_VALUE) if st else (None, None)


def _to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


# ---- forward --------------------------------------------------------------------------------------------------------------------
def _fwd(H, M, res=True, sum=True, p=0.0, pp=0.0, rps=0, st=False, eps=1e-12, dgb=False):
    return dict(H=H, M=M, res=res, sum=sum, p=p, pp=pp, rps=rps, st=st, eps=eps, dgb=dgb)


# every NCH and every M of {1, 3, 4, 5: wave and workgroup edges; 4096, 4097, 4101, 8193: the 1024-workgroup cap with one, two
# and three trips and a ragged last trip}
FWD_CASES = [
    _fwd(256, 1),
    _fwd(256, 4097, res=False, p=0.1, eps=1e-6),
    _fwd(256, 8193, sum=False, dgb=True),
    _fwd(512, 3, res=False, sum=False),
    _fwd(512, 4096, pp=0.3, rps=7, eps=1e-6),
    _fwd(512, 4101, p=0.1, pp=0.3, rps=1, st=True),
    _fwd(768, 4, sum=False, p=0.1),
    _fwd(768, 5, res=False, p=0.1, st=True, eps=1e-6),
    _fwd(768, 4101, pp=0.3, rps=7, dgb=True, eps=1e-6),
    _fwd(768, 8193, p=0.1),
    _fwd(1024, 5, pp=0.3, rps=1),
    _fwd(1024, 4097, sum=False, p=0.1, eps=1e-6),
    _fwd(1024, 8193, res=False),
]


@pytest.mark.parametrize("c", FWD_CASES, ids=_case_id)
def test_forward(dev, ext, c):
    H, M = c["H"], c["M"]
    d = R.inputs(M, H)
    res = d["res"] if c["res"] else None
    st, sv = _seed_args(dev, c["st"])
    kscale, ps = R.masks(M, H, c["p"], c["pp"], c["rps"], SEED, sv)
    ref = R.forward(d["x"], res, d["gamma"], d["beta"], c["eps"], kscale, ps)
    x, r, g, b = _to(dev, d["x"], res, d["gamma"], d["beta"])
    y, s, mean, rstd, dgb = ext.drop_add_ln_fwd(x, r, g, b, c["eps"], c["p"], SEED, st, c["sum"], c["pp"], c["rps"], c["dgb"])
    hold = _Hold(_case_id(c))
    hold("y", y, ref["y"], ref["tol_y"])
    hold.true(mean.shape == (M,) and rstd.shape == (M,) and bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all()),
              "mean / rstd not finite for every row")
    hold("mean", mean, ref["mean"], ref["tol_mean"])
    hold("rstd", rstd, ref["rstd"], ref["tol_rstd"])
    hold.true((s is not None) == c["sum"] and (dgb is not None) == c["dgb"], "optional outputs")
    if dgb is not None:
        hold.true(dgb.shape == (2, H) and bool((dgb.view(torch.int32) == 0).all()), "the dgamma / dbeta accumulator is not exactly zero")
    if s is not None:
        hold("sum", s, ref["z"], ref["tol_sum"])
        sc = s.cpu()
        if ps is not None and res is not None:
            dropped = ps == 0
            hold.true(M < 64 or (bool(dropped.any()) and not bool(dropped.all())), "the path mask drops none or all")
            hold.true(torch.equal(_bits(sc[dropped]), _bits(res[dropped])), "a dropped sample's sum is not its residual bit for bit")
        if kscale is not None and res is None and ps is None:
            hold.true(torch.equal(sc == 0, kscale == 0), "the elements with sum == 0 are not the ones the CPU keep mask drops")
    hold.assert_ok()


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _bwd(H, M, form="x", res=True, dsum=True, p=0.0, pp=0.0, rps=0, st=False):
    return dict(H=H, M=M, form=form, res=res, dsum=dsum, p=p, pp=pp, rps=rps, st=st)


# M: 1, 5 and the 384-workgroup cap with one (1536), two (1537, 1541) and three (3077) trips
BWD_CASES = [
    _bwd(256, 1),
    _bwd(256, 1541, res=False, dsum=False, p=0.1),
    _bwd(256, 3077, form="sum", pp=0.3, rps=7),
    _bwd(512, 5, dsum=False, p=0.1, pp=0.3, rps=1),
    _bwd(512, 1536, form="sum", dsum=False),
    _bwd(512, 1537, pp=0.3, rps=7),
    _bwd(768, 5, form="sum"),
    _bwd(768, 1541, p=0.1, pp=0.3, rps=7, st=True),
    _bwd(768, 3077, dsum=False, p=0.1),
    _bwd(1024, 1, res=False),
    _bwd(1024, 1537, form="sum", pp=0.3, rps=1),
    _bwd(1024, 3077),
]
EPS_B = 1e-6


def _bwd_setup(c, sv):
    """the CPU operands of a backward case: (x or the stored sum, res, dsum, kscale, ps, mean, rstd), statistics in fp64
    rounded once to fp32"""
    H, M = c["H"], c["M"]
    d = R.inputs(M, H)
    kscale, ps = R.masks(M, H, c["p"], c["pp"], c["rps"], SEED, sv)
    dsum = d["dsum"] if c["dsum"] else None
    if c["form"] == "sum":
        z = R.forward(d["x"], d["res"], d["gamma"], d["beta"], EPS_B, None, ps)["z"]
        xin, res, kscale = z.to(torch.bfloat16), None, None
        m32, r32 = R.stats32(xin.double(), EPS_B)
    else:
        res = d["res"] if c["res"] else None
        xin = d["x"]
        m32, r32 = R.stats32(R.forward(xin, res, d["gamma"], d["beta"], EPS_B, kscale, ps)["z"], EPS_B)
    return d, xin, res, dsum, kscale, ps, m32, r32


def _run_bwd(ext, dev, c, d, xin, res, dsum, m32, r32, st):
    x, r, g, dy, ds, m, rs = _to(dev, xin, res, d["gamma"], d["dy"], dsum, m32, r32)
    if c["form"] == "sum":
        return ext.drop_add_ln_bwd_sum(x, g, dy, m, rs, EPS_B, SEED, st, ds, c["pp"], c["rps"])
    return ext.drop_add_ln_bwd(x, r, g, dy, m, rs, EPS_B, c["p"], SEED, st, ds, c["pp"], c["rps"])


def _hold_bwd(hold, c, ref, out, res):
    dx, dres, dg, db = out
    hold("dx", dx, ref["dx"], ref["tol_dx"])
    hold.true(bool((dx.cpu()[ref["dropped"]] == 0).all()), "dx is not exactly 0 where the mask or the path drops")
    if c["form"] == "sum" and c["pp"] == 0:
        hold.true(dres is dx, "the stored-sum form without stochastic depth must return ONE tensor for dx and dres")
    elif c["form"] == "x" and res is None:
        hold.true(dres is None, "dres without a residual")
    else:
        hold("dres", dres, ref["dz"], ref["tol_dres"])
    hold("dgamma", dg, ref["dgamma"], ref["tol_dgamma"])
    hold("dbeta", db, ref["dbeta"], ref["tol_dbeta"])


@pytest.mark.parametrize("c", BWD_CASES, ids=_case_id)
def test_backward(dev, ext, c):
    st, sv = _seed_args(dev, c["st"])
    d, xin, res, dsum, kscale, ps, m32, r32 = _bwd_setup(c, sv)
    ref = R.backward(xin, res, d["gamma"], d["dy"], dsum, m32, r32, kscale, ps, c["form"] == "sum")
    hold = _Hold(_case_id(c))
    _hold_bwd(hold, c, ref, _run_bwd(ext, dev, c, d, xin, res, dsum, m32, r32, st), res)
    hold.assert_ok()


@pytest.mark.parametrize("form", ["x", "sum"])
def test_backward_chained_to_the_kernels_own_forward(dev, ext, form):
    """the kernel's own mean, rstd (and stored sum) go into its backward and into the reference"""
    M, H = 1541, 768
    c = _bwd(H, M, form=form, p=0.1 if form == "x" else 0.0, pp=0.3, rps=7)
    d = R.inputs(M, H)
    kscale, ps = R.masks(M, H, c["p"], c["pp"], c["rps"], SEED)
    x, r, g, b, dy, ds = _to(dev, d["x"], d["res"], d["gamma"], d["beta"], d["dy"], d["dsum"])
    y, s, mean, rstd, dgb = ext.drop_add_ln_fwd(x, r, g, b, EPS_B, c["p"], SEED, None, True, c["pp"], c["rps"], True)
    hold = _Hold("chained-" + form)
    if form == "sum":
        out = ext.drop_add_ln_bwd_sum(s, g, dy, mean, rstd, EPS_B, SEED, None, ds, c["pp"], c["rps"], dgb)
        ref = R.backward(s.cpu(), None, d["gamma"], d["dy"], d["dsum"], mean.cpu(), rstd.cpu(), None, ps, True)
    else:
        out = ext.drop_add_ln_bwd(x, r, g, dy, mean, rstd, EPS_B, c["p"], SEED, None, ds, c["pp"], c["rps"], dgb)
        ref = R.backward(d["x"], d["res"], d["gamma"], d["dy"], d["dsum"], mean.cpu(), rstd.cpu(), kscale, ps)
    hold.true(out[2].data_ptr() == dgb.data_ptr(), "dgamma is not the accumulator the forward zeroed")
    _hold_bwd(hold, c, ref, out, d["res"])
    hold.assert_ok()


# ---- two row groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,p", [(2, 256, 0.1), (10, 768, 0.0), (2 * 1541, 1024, 0.1), (2 * 4099, 512, 0.0)])
def test_twin(dev, ext, M, H, p):
    """each group's rows and each group's dgamma / dbeta slice against the bound computed with that group's parameters"""
    d = R.inputs(M, H)
    Mg = M // 2
    kscale, _ = R.masks(M, H, p, 0.0, 0, SEED)
    x, r, g, b, g2, b2, dy = _to(dev, d["x"], d["res"], d["gamma"], d["beta"], d["gamma2"], d["beta2"], d["dy"])
    y, mean, rstd, dgb = ext.twin_drop_add_ln_fwd(x, r, g, b, g2, b2, 1e-12, p, SEED, None, True)
    hold = _Hold("twin-%d-%d-%g" % (M, H, p))
    hold.true(dgb.shape == (2, 2, H) and bool((dgb.view(torch.int32) == 0).all()), "the (2, 2, H) accumulator is not exactly zero")
    m32 = r32 = None
    for grp, (gg, bb) in enumerate(((d["gamma"], d["beta"]), (d["gamma2"], d["beta2"]))):
        rows = slice(grp * Mg, (grp + 1) * Mg)
        ks = kscale[rows] if kscale is not None else None
        ref = R.forward(d["x"][rows], d["res"][rows], gg, bb, 1e-12, ks)
        hold("y", y[rows], ref["y"], ref["tol_y"], "y group %d" % grp)
        hold("mean", mean[rows], ref["mean"], ref["tol_mean"], "mean group %d" % grp)
        hold("rstd", rstd[rows], ref["rstd"], ref["tol_rstd"], "rstd group %d" % grp)
        m, rs = R.stats32(ref["z"], 1e-12)
        m32, r32 = (m, rs) if grp == 0 else (torch.cat([m32, m]), torch.cat([r32, rs]))
    dx, dres, dgb = ext.twin_drop_add_ln_bwd(x, r, g, g2, dy, m32.to(dev), r32.to(dev), 1e-12, p, SEED, None, dgb)
    hold.true(dgb.shape == (2, 2, H), "dgb shape")
    for grp, gg in enumerate((d["gamma"], d["gamma2"])):
        rows = slice(grp * Mg, (grp + 1) * Mg)
        ks = kscale[rows] if kscale is not None else None
        ref = R.backward(d["x"][rows], d["res"][rows], gg, d["dy"][rows], None, m32[rows], r32[rows], ks)
        hold("dx", dx[rows], ref["dx"], ref["tol_dx"], "dx group %d" % grp)
        hold.true(bool((dx[rows].cpu()[ref["dropped"]] == 0).all()), "dx not 0 where the mask drops, group %d" % grp)
        hold("dres", dres[rows], ref["dz"], ref["tol_dres"], "dres group %d" % grp)
        hold("dgamma", dgb[grp, 0], ref["dgamma"], ref["tol_dgamma"], "dgamma group %d" % grp)
        hold("dbeta", dgb[grp, 1], ref["dbeta"], ref["tol_dbeta"], "dbeta group %d" % grp)
    hold.assert_ok()


def test_twin_rejects_an_odd_row_count(dev, ext):
    d = R.inputs(3, 256)
    x, r, g, b, g2, b2, dy = _to(dev, d["x"], d["res"], d["gamma"], d["beta"], d["gamma2"], d["beta2"], d["dy"])
    with pytest.raises(RuntimeError, match="bad row groups"):
        ext.twin_drop_add_ln_fwd(x, r, g, b, g2, b2, 1e-12, 0.0, SEED, None)
    ones = torch.ones(3, device=dev)
    with pytest.raises(RuntimeError, match="bad row groups"):
        ext.twin_drop_add_ln_bwd(x, r, g, g2, dy, ones, ones, 1e-12, 0.0, SEED, None)


# ---- the deterministic mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [_bwd(768, 5, p=0.1), _bwd(768, 1541, p=0.1, pp=0.3, rps=7), _bwd(768, 5, form="sum"),
                               _bwd(768, 1541, form="sum", pp=0.3, rps=7)], ids=_case_id)
def test_backward_deterministic_mode(dev, ext, c):
    """the same bounds; two runs bit-equal in all four outputs; dx and dres bit-equal to the default mode's (the same kernel
    body: DET changes only where the dgamma / dbeta partials are stored)"""
    import bridgeqa_amd
    d, xin, res, dsum, kscale, ps, m32, r32 = _bwd_setup(c, None)
    ref = R.backward(xin, res, d["gamma"], d["dy"], dsum, m32, r32, kscale, ps, c["form"] == "sum")
    run = lambda: _run_bwd(ext, dev, c, d, xin, res, dsum, m32, r32, None)
    off = run()
    prev = bridgeqa_amd.set_deterministic(True)
    try:
        on, again = run(), run()
    finally:
        bridgeqa_amd.set_deterministic(prev)
    hold = _Hold("det-" + _case_id(c))
    _hold_bwd(hold, c, ref, on, res)
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), on, again):
        hold.true(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                              b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), "%s differs between two runs" % name)
    hold.true(torch.equal(_bits(on[0]), _bits(off[0])) and torch.equal(_bits(on[1]), _bits(off[1])),
              "dx / dres differ from the default mode's")
    hold.assert_ok()


# ---- rejected arguments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [384, 1280])
def test_unsupported_width_raises(dev, ext, H):
    x = torch.zeros(4, H, dtype=torch.bfloat16, device=dev)
    g, v = torch.ones(H, device=dev), torch.ones(4, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.drop_add_ln_fwd(x, x, g, g, 1e-6, 0.0, SEED, None)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.drop_add_ln_bwd(x, x, g, x, v, v, 1e-6, 0.0, SEED, None)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.drop_add_ln_bwd_sum(x, g, x, v, v, 1e-6, SEED, None)


def test_no_rows(dev, ext):
    H = 768
    x = torch.zeros(0, H, dtype=torch.bfloat16, device=dev)
    g, v = torch.ones(H, device=dev), torch.ones(0, device=dev)
    y, s, mean, rstd, dgb = ext.drop_add_ln_fwd(x, x, g, g, 1e-6, 0.1, SEED, None, True, 0.0, 0, True)
    assert y.shape == (0, H) and s.shape == (0, H) and mean.shape == (0,) and rstd.shape == (0,)
    assert dgb.shape == (2, H) and not bool(dgb.any())
    dx, dres, dg, db = ext.drop_add_ln_bwd(x, x, g, x, v, v, 1e-6, 0.1, SEED, None, None, 0.0, 0, dgb)
    assert dx.shape == (0, H) and dres.shape == (0, H) and not bool(dg.any()) and not bool(db.any())


# ---- GELU -----------------------------------------------------------------------------------------------------------------------
def test_gelu_every_finite_bf16_value(dev, ext):
    """all 65280 finite bit patterns, tiled 129 times: 8.42 M elements, more than the 4096 workgroups x 256 lanes x 8 of one
    trip of the grid-stride loop, so the last 4064 vectors are a second trip's"""
    pat = R.finite_bf16_patterns()
    r, tol = R.gelu_bound(pat)
    reps = 129
    assert pat.numel() * reps > 4096 * 256 * 8 and pat.numel() * reps % 8 == 0
    x = pat.repeat(reps).to(dev)
    y = ext.gelu_fwd(x).cpu()
    hold = _Hold("gelu")
    hold.true(y.dtype == torch.bfloat16 and y.shape == x.shape and bool(torch.isfinite(y.float()).all()), "not finite")
    hold("gelu", y, r.repeat(reps), tol.repeat(reps))
    zeros = (pat.float() == 0).repeat(reps)
    hold.true(int(zeros.sum()) == 2 * reps and bool((y[zeros].float() == 0).all()), "gelu(+-0) is not 0")
    hold.assert_ok()


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_gelu_short_tensors(dev, ext, n):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 3).to(torch.bfloat16)
    r, tol = R.gelu_bound(x)
    hold = _Hold("gelu-%d" % n)
    hold("gelu", ext.gelu_fwd(x.to(dev)), r, tol)
    hold.assert_ok()


def test_gelu_rejects_a_length_that_is_no_multiple_of_8(dev, ext):
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.gelu_fwd(torch.zeros(12, dtype=torch.bfloat16, device=dev))
