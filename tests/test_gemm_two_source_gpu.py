"""The second contraction segment of the 256 x 256 weight-gradient kernel (csrc/gemm.hip, BQ_GEMM_SECOND; _ext.gemm_grouped
problem keys P2 / Q2): dW = Qa^T Pa + Qb^T Pb in one launch, and the deferred flush that uses it (fusion_wgrad.py).

Both tiers of tests/gemm_ref.py: small-integer operands must give the integer result with == (the fp32 sum is exact in any
order, so a dropped or doubled K tile, a wrong row map or a K tile shared by the two segments is a wrong integer), real
operands stay within the per-element fp64 bound.  The logical problem is ONE contraction over ra + rb rows: P (Ni, ra + rb),
Q (Nj, ra + rb) of gemm_ref.operands, stored as two row sources.  Every buffer the kernel reads or writes is framed in NaN:
the gaps of the batched-row view, the rows before and behind every operand, the elements around out and colsum.

Shapes (the smallest at which each mechanism can fail): out 136 x 264 and 264 x 136 (a full and a ragged 256-tile along i,
then along j); primary rows 64 (one whole K tile) and 130 (two, ragged end); second source (3, 27, N)[:, 7:] = 60 rows, less than
one K tile, batches that cross the 8-row DMA groups; 128 rows (two whole K tiles) plain and as (8, 23, N)[:, 7:] batches of 16;
(16, 27, N)[:, 7:] = 320 rows, the twin K/V case, batches of 20 that fill five K tiles exactly (128 is no multiple of 20)."""
import ctypes
import math

import pytest
import torch

import gemm_ref as R
from gemm_ref import EPI_BIAS, EPI_NONE, OUT_F32, P_XC, Q_XC

pytestmark = pytest.mark.gpu

NAN = math.nan
DW = P_XC | Q_XC | OUT_F32
K256 = "gemm256_kernel<1,1,0,1,0>"
# second sources: (batches, rows per batch in the buffer, first row of the view) or the number of plain rows
SECOND = {"view60": (3, 27, 7), "view128": (8, 23, 7), "view320": (16, 27, 7), "rows128": 128}


def _rows_of(second):
    s = SECOND[second]
    return s if isinstance(s, int) else s[0] * (s[1] - s[2])


def _framed(X, dev, pad):
    """X (rows, cols) as a view inside a NaN buffer: `pad` gap columns, one row before and one behind"""
    r, c = X.shape
    buf = torch.full((r + 2, c + pad), NAN, dtype=X.dtype, device=dev)
    v = buf[1:1 + r, :c]
    v.copy_(X)
    return buf, v


def _frame_intact(buf, view):
    r, c = view.shape
    return int(torch.isnan(buf).sum()) == buf.numel() - r * c and not bool(torch.isnan(buf[1:1 + r, :c]).any())


def _second_q(Qb_t, second, dev):
    """Qb_t: (rb, Nj) rows of the second source -> the tensor handed to the kernel (a batched-row view inside a NaN buffer)"""
    s = SECOND[second]
    if isinstance(s, int):
        return _framed(Qb_t, dev, 8)[1]
    B, L, first = s
    buf = torch.full((B, L, Qb_t.shape[1]), NAN, dtype=Qb_t.dtype, device=dev)
    v = buf[:, first:]
    v.copy_(Qb_t.view(B, L - first, -1))
    return v


@pytest.fixture(scope="module")
def ext():
    from bridgeqa_amd import _ext
    return _ext


def _profiled(fn):
    """fn() under torch.profiler: the GEMM kernel ids it launched (the launch record of tests/test_gemm_bound_gpu.py)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    assert names, "the profiler reported no device kernels"
    return R.kernel_ids(names)


def _build(Ni, Nj, ra, second, colsum, exact, dev, tag=0):
    """one problem dict and what checks it.  second = None: an ordinary one-source problem"""
    rb = _rows_of(second) if second else 0
    P, Q, _, _ = (t.to(dev) for t in R.operands(Ni, Nj, ra + rb, exact, tag))
    pr = dict(P=_framed(P[:, :ra].t().contiguous(), dev, 8)[1], Q=_framed(Q[:, :ra].t().contiguous(), dev, 8)[1])
    if second:
        pr["P2"] = _framed(P[:, ra:].t().contiguous(), dev, 8)[1]
        pr["Q2"] = _second_q(Q[:, ra:].t().contiguous(), second, dev)
    obuf, pr["out"] = _framed(torch.full((Nj, Ni), NAN, dtype=torch.float32, device=dev), dev, 4)
    csbuf = None
    if colsum:
        csbuf = torch.full((Nj + 16,), NAN, device=dev)
        pr["colsum"] = csbuf[8:8 + Nj]
    return pr, (P, Q, obuf, csbuf)


def _check(pr, held, exact, name):
    P, Q, obuf, csbuf = held
    out = pr["out"]
    assert _frame_intact(obuf, out), "%s: a store left the logical output or missed an element" % name
    if exact:
        assert R.conditions(P, Q) < 2 ** 24
        bad = R.mismatches(out, R.expected(P, Q, f32=True))
        assert bad.shape[0] == 0, "%s: EXACT tier: %d of %d outputs differ, first at %s" % (
            name, bad.shape[0], out.numel(), tuple(int(v) for v in bad[0]))
    else:
        r, tol = R.bound(P, Q, f32=True)
        err = (out.double() - r).abs()
        assert bool((err <= tol).all()), "%s: BOUND tier: max |err| / tol = %.3g" % (name, float((err / tol).max()))
    if csbuf is not None:
        Nj = Q.shape[0]
        cs = csbuf[8:8 + Nj]
        assert bool(torch.isnan(csbuf[:8]).all()) and bool(torch.isnan(csbuf[8 + Nj:]).all()) and not bool(torch.isnan(cs).any()), \
            "%s: the canaries around colsum" % name
        r, tol = R.qsum_bound(Q)
        if exact:
            assert bool((cs.double() == r).all()), "%s: EXACT tier: column sums differ" % name
        else:
            assert bool(((cs.double() - r).abs() <= tol).all()), "%s: BOUND tier: column sums" % name


@pytest.mark.parametrize("colsum", [False, True], ids=["plain", "colsum"])
@pytest.mark.parametrize("second", sorted(SECOND))
@pytest.mark.parametrize("ra", [64, 130])
@pytest.mark.parametrize("Ni, Nj", [(264, 136), (136, 264)])
def test_two_sources_one_launch(ext, dev, Ni, Nj, ra, second, colsum):
    for exact in (True, False):
        pr, held = _build(Ni, Nj, ra, second, colsum, exact, dev)
        if exact:
            ids = _profiled(lambda: ext.gemm_grouped([pr], DW, EPI_NONE, 256))
            assert ids == {K256}, ids
        else:
            ext.gemm_grouped([pr], DW, EPI_NONE, 256)
            torch.cuda.synchronize()
        _check(pr, held, exact, "%dx%d ra=%d %s %s" % (Ni, Nj, ra, second, "int" if exact else "real"))


def test_continuation_entries_own_no_tiles(ext, dev):
    """two two-source problems around one ordinary problem in ONE launch: the tile accounting skips the continuation entries"""
    for exact in (True, False):
        built = [_build(264, 136, 130, "view60", True, exact, dev, tag=1), _build(136, 264, 64, None, True, exact, dev, tag=2),
                 _build(264, 136, 64, "view320", False, exact, dev, tag=3)]
        ids = _profiled(lambda: ext.gemm_grouped([b[0] for b in built], DW, EPI_NONE, 256))
        assert ids == {K256}, ids
        for k, (pr, held) in enumerate(built):
            _check(pr, held, exact, "mixed[%d].%s" % (k, "int" if exact else "real"))


def test_more_pairs_than_a_table_holds_split_into_launches(ext, dev):
    """19 two-source problems: 38 table entries against 36 -- the list is cut BETWEEN pairs"""
    assert ext._lib.bq_gemm_max_problems() == R.MAX_PROBLEMS
    built = [_build(136, 136, 64, "view60", k % 2 == 0, True, dev, tag=k % 3) for k in range(R.MAX_PROBLEMS // 2 + 1)]
    ext.gemm_grouped([b[0] for b in built], DW, EPI_NONE, 256)
    torch.cuda.synchronize()
    for k, (pr, held) in enumerate(built):
        _check(pr, held, True, "split[%d]" % k)


def test_second_source_is_refused_elsewhere(ext, dev):
    pr, _ = _build(264, 136, 130, "view60", False, True, dev)
    for tile in (128, 64):                                           # tile 256 only
        with pytest.raises(RuntimeError):
            ext.gemm_grouped([pr], DW, EPI_NONE, tile)
    with pytest.raises(RuntimeError):                                # no cut contraction
        ext.gemm_grouped([dict(pr, ksplit=2)], DW, EPI_NONE, 256)
    with pytest.raises(RuntimeError):                                # still no accum on tile 256
        ext.gemm_grouped([dict(pr, accum=True)], DW, EPI_NONE, 256)
    other, _ = _build(264, 144, 130, "view60", False, True, dev)     # the same Ni / Nj for both segments
    with pytest.raises(RuntimeError):
        ext.gemm_grouped([dict(pr, Q2=other["Q2"])], DW, EPI_NONE, 256)
    with pytest.raises(RuntimeError):
        ext.gemm_grouped([dict(pr, P2=_framed(torch.zeros(60, 272, dtype=torch.bfloat16, device=dev), dev, 8)[1])], DW, EPI_NONE, 256)
    with pytest.raises(RuntimeError):                                # both operands or none
        ext.gemm_grouped([{k: v for k, v in pr.items() if k != "P2"}], DW, EPI_NONE, 256)
    # fp32 output, P_XC | Q_XC, EPI_NONE only: the same buffers under other flags / epilogues (bf16 out where the form has one)
    ob = torch.zeros(136, 264, dtype=torch.bfloat16, device=dev)
    for flags, epi, out in ((P_XC | Q_XC, EPI_NONE, ob), (P_XC, EPI_NONE, ob), (DW, EPI_BIAS, pr["out"])):
        with pytest.raises(RuntimeError):
            ext.gemm_grouped([dict(pr, out=out)], flags, epi, 256)
    torch.cuda.synchronize()
    # the library itself (the checks above partly end in _ext): status, not a launch
    arr = (ext._GemmDesc * 2)()
    for k, (p, q) in enumerate(((pr["P"], pr["Q"]), (pr["P2"], pr["Q2"]))):
        arr[k].P, arr[k].Q = p.data_ptr(), q.data_ptr()
        arr[k].ldp, arr[k].ldq, arr[k].Ni, arr[k].Nj, arr[k].Kc = p.stride(0), q.stride(-2), 264, 136, p.shape[0]
    arr[0].out, arr[0].ldo = pr["out"].data_ptr(), pr["out"].stride(0)
    arr[1].q_rpb, arr[1].q_bstride = 20, pr["Q2"].stride(0)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda a, n, flags, epi, tile: ext._lib.bq_gemm_bf16(a, n, flags, epi, tile, ctypes.c_void_p(st))
    assert call(arr, 2, DW, EPI_NONE, 256) == -1                     # without BQ_GEMM_SECOND an entry without out is a null operand
    assert call(arr, 2, DW | ext.GEMM_SECOND, EPI_NONE, 64) == -1
    assert call(arr, 2, DW | ext.GEMM_SECOND, EPI_NONE, 128) == -1
    assert call(arr, 2, P_XC | ext.GEMM_SECOND, EPI_NONE, 256) == -1
    arr[1].Nj = 144
    assert call(arr, 2, DW | ext.GEMM_SECOND, EPI_NONE, 256) == -1
    arr[1].Nj, arr[1].Kc = 136, 50                                   # not whole batches of 20
    assert call(arr, 2, DW | ext.GEMM_SECOND, EPI_NONE, 256) == -1
    arr[1].Kc = 60
    orphan = (ext._GemmDesc * 2)(arr[1], arr[0])                     # a second source in front of its primary
    assert call(orphan, 2, DW | ext.GEMM_SECOND, EPI_NONE, 256) == -1
    assert b"gemm" in ext._lib.bq_last_error()
    pr["out"].fill_(NAN)
    assert call(arr, 2, DW | ext.GEMM_SECOND, EPI_NONE, 256) == 0    # and the same array, whole again, runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(pr["out"]).any())


# ---- the deferred flush ----------------------------------------------------------------------------------------------------
def test_flush_sums_a_parked_pair_in_the_256_tile_launch(ext, dev):
    """fusion_wgrad._park_two at the twin K/V node's layout: gradient (B, L1 + 20, N), the primary reads [:, :L1] (B x L1 = 1024
    rows: class big), the second source [:, L1:] in place.  The flush gives the gradient of fp32 torch within the bound and
    launches no 64-tile kernel for it."""
    from bridgeqa_amd import fusion_wgrad as W
    B, L1, L2, N, D = 16, 64, 20, 136, 264
    ra, rb = B * L1, B * L2
    assert W.wgrad_class(ra) == "big"
    for exact in (True, False):
        P, Q, _, _ = (t.to(dev) for t in R.operands(D, N, ra + rb, exact, 5))
        g = torch.full((B, L1 + L2, N), NAN, dtype=torch.bfloat16, device=dev)
        g[:, :L1] = Q[:, :ra].t().reshape(B, L1, N)
        g[:, L1:] = Q[:, ra:].t().reshape(B, L2, N)
        xa, xb = P[:, :ra].t().contiguous(), P[:, ra:].t().contiguous()
        ws = [torch.nn.Parameter(torch.zeros(N // 2, D, device=dev)) for _ in range(2)]
        bs = [torch.nn.Parameter(torch.zeros(N // 2, device=dev)) for _ in range(2)]
        W.begin_deferred_wgrad()
        W._park_two(g[:, :L1], xa, g[:, L1:], xb, ws, bs)
        items = W.take_deferred_wgrad()
        ids = _profiled(lambda: W.flush_deferred_items(items))
        assert ids == {K256}, ids
        dw, db = torch.cat([w.grad for w in ws]), torch.cat([b.grad for b in bs])
        want_w = Q.float() @ P.float().t()                       # the gradient of fp32 torch: dW = dY^T X over both sources
        if exact:
            assert torch.equal(dw, want_w) and bool((db.double() == Q.double().sum(1)).all())
        else:
            r, tol = R.bound(P, Q, f32=True)
            assert bool(((dw.double() - r).abs() <= tol).all())
            assert bool(((dw.double() - want_w.double()).abs() <= 2 * tol).all())   # (torch's own fp32 sum errs within the same bound)
            r, tol = R.qsum_bound(Q)
            assert bool(((db.double() - r).abs() <= tol).all())
