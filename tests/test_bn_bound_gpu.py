"""The training-mode BatchNorm kernels of csrc/bn.hip (bn_stats_kernel, bn_finalize_kernel, bn_fold_kernel, the four
bn_apply_kernel, bn_bwd_reduce_kernel and bn_bwd_dx_kernel forms) and bn_bwd_reduce_arg_kernel of csrc/detbwd.hip held to the
per-element fp64 bounds of tests/bn_ref.py: a dropped row, phase or partial, a later maximum, a non-strict ReLU mask, a wrong
divisor, two swapped channels or one wrong arg byte fails, where the whole-tensor norms of tests/test_modules_gpu.py accept it.
Every case calls the _ext wrappers directly, moves the results to the CPU and compares every element; `not (err <= tol)` fails,
so NaN fails; every arg table must equal the reference byte for byte.

The apply and backward cases take mean and rstd computed in fp64 and rounded once to fp32, scale and shift formed from these
and rounded once (bn_ref.given_stats), so that a defect of the statistics cannot hide one of the later passes; the chained
cases feed the kernel's own statistics into its apply and backward and into the reference instead.

Which edge each case reaches is said at the case lists of tests/bn_ref.py.  The largest |err| / bound per output kind is printed
at the end of the module (pytest -s); on an MI355X:
    mean 0.337  rstd 0.306  scale 0.35  shift 0.278  running_mean 0.347  running_var 0.358
    y 0.996  y_pool 0.996  dx 0.996  dgamma 0.19  dbeta 0.0217  dgamma_arg 0.159  dbeta_arg 0.00913
-- the bf16 outputs sit just below 1 because round-to-nearest reaches 2^-8 relative just above a power of two; every arg table
equalled the reference byte for byte, and no kernel needed a change.
"""
import pytest
import torch

import bn_ref as B

pytestmark = pytest.mark.gpu

_WORST = {}
EPS = 1e-5


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
        ratio, msg = B.excess(out, ref, tol)
        _WORST[kind] = max(_WORST.get(kind, 0.0), ratio)
        if msg:
            self.fails.append("%s %s: %s" % (self.name, what or kind, msg))

    def true(self, cond, msg):
        if not cond:
            self.fails.append("%s: %s" % (self.name, msg))

    def assert_ok(self):
        assert not self.fails, "\n".join(self.fails)


def _to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


def _apply_arg(ext, x, st, S, relu, pool):
    """bq_bn_apply_arg through the signature _ext declares for it: (out, arg), arg u8 of out's shape.  _ext has no wrapper that
    hands the table out on its own (bn_apply passes no table; pwconv_bn_fwd fills one behind its GEMM), and bn_apply stays as it
    is here: it runs in every training step"""
    R, C = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty(R // S if pool else R, C, dtype=torch.bfloat16, device=x.device)
        arg = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
        ext._check(ext._lib.bq_bn_apply_arg(ext._p(x), ext._p(st[0]), ext._p(st[1]), ext._p(out), ext._p(arg), R, C, int(S),
                                            int(bool(relu)), int(bool(pool)), ext._stream()), "bn_apply")
    return out, arg


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- statistics -----------------------------------------------------------------------------------------------------------------
def _hold_stats(hold, st, ref):
    for i, k in enumerate(("scale", "shift", "mean", "rstd")):
        hold(k, st[i], ref[k], ref["tol_" + k])


@pytest.mark.parametrize("c", B.STATS_CASES, ids=B.case_id)
def test_statistics(dev, ext, c):
    """mean, rstd, scale, shift and the running buffers against the bound; y (ReLU, not pooled) against the reference built
    from the kernel's OWN scale and shift"""
    R, C = c["R"], c["C"]
    d = B.inputs(R, C)
    ref = B.stats(d["x"], d["gamma"], d["beta"], c["eps"], c["m"], d["rm"], d["rv"])
    x, g, b = _to(dev, d["x"], d["gamma"], d["beta"])
    rm, rv = (d["rm"].clone().to(dev), d["rv"].clone().to(dev)) if c["run"] else (None, None)
    nbt = torch.zeros((), dtype=torch.int64, device=dev) if c["run"] else None
    y, st = ext.bn_relu_fwd(x, g, b, rm, rv, nbt, c["eps"], c["m"], 1, True, False)
    hold = _Hold(B.case_id(c))
    hold.true(st.shape == (4, C) and st.dtype == torch.float32 and bool(torch.isfinite(st).all()), "statistics not finite")
    _hold_stats(hold, st, ref)
    if c["run"]:
        hold("running_mean", rm, ref["running_mean"], ref["tol_running_mean"])
        hold("running_var", rv, ref["running_var"], ref["tol_running_var"])
        hold.true(int(nbt) == 1, "num_batches_tracked %d after one call" % int(nbt))
    if R == 1:
        hold.true(bool((ref["var"] == 0).all()) and bool((ref["unbiased"] == 0).all()), "R = 1: the reference variance is not 0")
    a = B.apply(d["x"], st[0].cpu(), st[1].cpu(), 0, True, False)
    hold("y", y, a["y"], a["tol_y"])
    hold.assert_ok()


def test_statistics_two_calls_on_the_same_buffers(dev, ext):
    """num_batches_tracked == 2 and the two-step recurrence of the running buffers, the first step's bound carried along"""
    R, C, m = 300, 64, 0.1
    d = B.inputs(R, C)
    x, g, b, rm, rv = _to(dev, d["x"], d["gamma"], d["beta"], d["rm"].clone(), d["rv"].clone())
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(2):
        ext.bn_relu_fwd(x, g, b, rm, rv, nbt, EPS, m, 1, True, False)
    r1 = B.stats(d["x"], d["gamma"], d["beta"], EPS, m, d["rm"], d["rv"])
    r2 = B.stats(d["x"], d["gamma"], d["beta"], EPS, m, r1["running_mean"], r1["running_var"],
                 r1["tol_running_mean"], r1["tol_running_var"])
    hold = _Hold("two-calls")
    hold.true(int(nbt) == 2, "num_batches_tracked %d after two calls" % int(nbt))
    hold("running_mean", rm, r2["running_mean"], r2["tol_running_mean"])
    hold("running_var", rv, r2["running_var"], r2["tol_running_var"])
    hold.assert_ok()


# ---- apply ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.APPLY_CASES, ids=B.case_id)
def test_apply(dev, ext, c):
    """the four template forms with test-made statistics; the arg table byte for byte where it exists (S <= 256)"""
    R, C, S = c["R"], c["C"], c["S"]
    d = B.inputs(R, C, S)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    ref = B.apply(d["x"], st[0], st[1], S, c["relu"], c["pool"])
    x, std = _to(dev, d["x"], st)
    hold = _Hold(B.case_id(c))
    if c["arg"]:
        y, arg = _apply_arg(ext, x, std, S, c["relu"], c["pool"])
        hold.true(arg.dtype == torch.uint8 and arg.shape == (R // S, C), "the arg table's type or shape")
        wrong = arg.cpu() != ref["arg"]
        hold.true(not bool(wrong.any()), "%d arg bytes differ from the first maximum, first at %s" % (
            int(wrong.sum()), tuple(wrong.nonzero()[0].tolist()) if wrong.any() else None))
        if S >= 2 and R // S >= 50:
            hold.true(bool((ref["arg"][d["tied"]].long() < S - 1).any()), "no tied group in the case")
    else:
        y = ext.bn_apply(x, std, S, c["relu"], c["pool"])
    hold.true(y.dtype == torch.bfloat16 and y.shape == ref["y"].shape, "the output's type or shape")
    hold("y_pool" if c["pool"] else "y", y, ref["y"], ref["tol_y"])
    if c["relu"]:
        hold.true(bool((y.float() >= 0).all()), "a negative output under ReLU")
    hold.assert_ok()


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _hold_bwd(hold, out, ref):
    dx, dg, db = out
    hold("dx", dx, ref["dx"], ref["tol_dx"])
    hold("dgamma", dg, ref["dgamma"], ref["tol_dgamma"])
    hold("dbeta", db, ref["dbeta"], ref["tol_dbeta"])


@pytest.mark.parametrize("c", B.BWD_CASES, ids=B.case_id)
def test_backward(dev, ext, c):
    """bn_relu_bwd (reduce, fold, dx) with test-made statistics; dx on every row"""
    R, C, S = c["R"], c["C"], c["S"]
    d = B.inputs(R, C, S)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    ref = B.backward(d["dy"], d["x"], st, S, c["relu"], c["pool"])
    dy, x, std = _to(dev, d["dy"], d["x"], st)
    hold = _Hold(B.case_id(c))
    out = ext.bn_relu_bwd(dy, x, std, S, c["relu"], c["pool"])
    hold.true(out[0].shape == (R, C) and out[0].dtype == torch.bfloat16, "dx type or shape")
    _hold_bwd(hold, out, ref)
    dgb = ext.bn_bwd_reduce(dy, x, std, S, c["relu"], c["pool"])
    hold.true(torch.equal(_bits(dgb[1]), _bits(out[1])) and torch.equal(_bits(dgb[0]), _bits(out[2])),
              "bn_bwd_reduce and bn_relu_bwd differ in dgamma / dbeta (the same kernels)")
    hold.assert_ok()


@pytest.mark.parametrize("c", B.TABLE_CASES, ids=B.case_id)
def test_table_reading_reduce(dev, ext, c):
    """bn_bwd_reduce(..., arg = the reference's table): the same dgamma / dbeta bound at the table kernel's own depth"""
    R, C, S = c["R"], c["C"], c["S"]
    d = B.inputs(R, C, S)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    ref = B.backward(d["dy"], d["x"], st, S, c["relu"], True)
    table = ref["arg"].to(torch.uint8)
    assert int(table.max()) < S and table.shape == (R // S, C) and "tol_dgamma_arg" in ref
    dy, x, std, arg = _to(dev, d["dy"], d["x"], st, table)
    dgb = ext.bn_bwd_reduce(dy, x, std, S, c["relu"], True, arg=arg)
    hold = _Hold(B.case_id(c))
    hold("dgamma_arg", dgb[1], ref["dgamma"], ref["tol_dgamma_arg"])
    hold("dbeta_arg", dgb[0], ref["dbeta"], ref["tol_dbeta_arg"])
    hold.assert_ok()


# ---- chained ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,S", [(16 * 529, 64, 16), (1500, 64, 0)], ids=["pooled", "unpooled"])
def test_chained_to_the_kernels_own_statistics(dev, ext, R, C, S):
    """the kernel's own scale, shift, mean, rstd go into its apply and backward AND into the reference as given values"""
    pool = S > 0
    d = B.inputs(R, C, S)
    fref = B.stats(d["x"], d["gamma"], d["beta"], EPS, 0.1)
    dy, x, g, b = _to(dev, d["dy"], d["x"], d["gamma"], d["beta"])
    y, st = ext.bn_relu_fwd(x, g, b, None, None, None, EPS, 0.1, max(S, 1), True, pool)
    stc = st.cpu()
    hold = _Hold("chained-%d" % S)
    _hold_stats(hold, st, fref)
    a = B.apply(d["x"], stc[0], stc[1], S, True, pool)
    hold("y_pool" if pool else "y", y, a["y"], a["tol_y"])
    if pool:
        y2, arg = _apply_arg(ext, x, st, S, True, True)
        hold.true(torch.equal(_bits(y2), _bits(y)), "bq_bn_apply_arg and bn_relu_fwd differ in y")
        hold.true(torch.equal(arg.cpu(), a["arg"]), "arg bytes differ from the first maximum")
    ref = B.backward(d["dy"], d["x"], stc, S, True, pool)
    _hold_bwd(hold, ext.bn_relu_bwd(dy, x, st, S, True, pool), ref)
    if pool:
        dgb = ext.bn_bwd_reduce(dy, x, st, S, True, True, arg=arg)
        hold("dgamma_arg", dgb[1], ref["dgamma"], ref["tol_dgamma_arg"])
        hold("dbeta_arg", dgb[0], ref["dbeta"], ref["tol_dbeta_arg"])
    hold.assert_ok()


# ---- reproducible -----------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal(dev, ext):
    """csrc/bn.hip: 'the fixed chunk order makes every result bit-reproducible'"""
    d = B.inputs(8453, 8)
    x, g, b = _to(dev, d["x"], d["gamma"], d["beta"])
    runs = [ext.bn_relu_fwd(x, g, b, None, None, None, EPS, 0.1, 1, True, False) for _ in range(2)]
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])) and torch.equal(_bits(runs[0][0]), _bits(runs[1][0]))
    R, C, S = 16 * 529, 64, 16
    d = B.inputs(R, C, S)
    st = B.given_stats(d["x"], d["gamma"], d["beta"], EPS)
    dy, x, std = _to(dev, d["dy"], d["x"], st)
    runs = [ext.bn_relu_bwd(dy, x, std, S, True, True) for _ in range(2)]
    for a, b2, name in zip(runs[0], runs[1], ("dx", "dgamma", "dbeta")):
        assert torch.equal(_bits(a), _bits(b2)), "%s differs between two runs" % name


# ---- rejected, before any launch --------------------------------------------------------------------------------------------------
def _ones_stats(C, dev):
    return torch.ones(4, C, device=dev)


@pytest.mark.parametrize("C", [24, 4096])
def test_unsupported_width_raises(dev, ext, C):
    x = torch.zeros(16, C, dtype=torch.bfloat16, device=dev)
    g, st = torch.ones(C, device=dev), _ones_stats(C, dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_relu_fwd(x, g, g, None, None, None, EPS, 0.1, 1, True, False)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_apply(x, st, 1, True, False)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_relu_bwd(x, x, st, 1, True, False)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_bwd_reduce(x, x, st, 1, True, False)


@pytest.mark.parametrize("R,S", [(48, 3), (4096, 2048), (40, 16)], ids=["S3", "S2048", "ragged"])
def test_unsupported_pooling_raises(dev, ext, R, S):
    C = 8
    x = torch.zeros(R, C, dtype=torch.bfloat16, device=dev)
    dy = torch.zeros(max(R // S, 1), C, dtype=torch.bfloat16, device=dev)
    st = _ones_stats(C, dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_apply(x, st, S, True, True)
    with pytest.raises(RuntimeError, match="unsupported"):
        _apply_arg(ext, x, st, S, True, True)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_relu_bwd(dy, x, st, S, True, True)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.bn_bwd_reduce(dy, x, st, S, True, True)


def test_the_arg_table_is_for_groups_of_at_most_256_rows(dev, ext):
    x = torch.zeros(1024, 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="S <= 256"):
        _apply_arg(ext, x, _ones_stats(8, dev), 512, True, True)
    with pytest.raises(RuntimeError, match="pooled"):
        _apply_arg(ext, x, _ones_stats(8, dev), 16, True, False)


def test_no_rows(dev, ext):
    C = 64
    x = torch.zeros(0, C, dtype=torch.bfloat16, device=dev)
    g = torch.ones(C, device=dev)
    with pytest.raises(RuntimeError, match="empty batch"):
        ext.bn_relu_fwd(x, g, g, None, None, None, EPS, 0.1, 1, True, False)
    y = ext.bn_apply(x, _ones_stats(C, dev), 1, True, False)
    assert y.shape == (0, C) and y.dtype == torch.bfloat16
    y, arg = _apply_arg(ext, x, _ones_stats(C, dev), 16, True, True)
    assert y.shape == (0, C) and arg.shape == (0, C) and arg.dtype == torch.uint8
