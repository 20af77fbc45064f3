"""GPU parity of the MFMA bf16 GEMM family (csrc/gemm.hip) against a plain torch fp32 composition of the same op
(the reference's nn.Linear and its autograd: models/vit.py:30-32,51-53; models/med.py:112-118,232,295,310).

Tolerances: operands are bf16 on both sides; the kernels accumulate in fp32 and round ONCE to bf16 (fp32 for weight
gradients), so an output differs from the fp32 reference by at most bf16 rounding: rel-L2 <= 3e-3 and
max |err| <= 1e-2 * max |ref| for bf16 outputs, rel-L2 <= 1e-5 for fp32 outputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(torch.bfloat16)


def _check(out, ref, f32=False):
    out, ref = out.float(), ref.float()
    assert torch.isfinite(out).all()
    rel = ((out - ref).norm() / (ref.norm() + 1e-20)).item()
    mx = ((out - ref).abs().max() / (ref.abs().max() + 1e-20)).item()
    assert rel <= (1e-5 if f32 else 3e-3), (rel, mx)
    assert mx <= (1e-4 if f32 else 1e-2), (rel, mx)


def _gelu(x):
    return torch.nn.functional.gelu(x)


FWD_SHAPES = [(1000, 512, 192), (256, 256, 64), (2100, 1024, 256), (16400, 768, 768), (257, 264, 128)]


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
@pytest.mark.parametrize("tile", [256, 128, 64, 32])
def test_forward_bias(dev, M, N, K, tile):
    from bridgeqa_amd import _ext
    if tile < 128 and M * N > 4e6:
        pytest.skip("small-tile kernels are for small problems")
    if tile == 128 and K < 128:
        pytest.skip("the 256 x 128 kernel's DMA stream runs two K tiles ahead: K >= 128")
    x, w = _rand((M, K), dev, 1), _rand((N, K), dev, 2, 0.1)
    b = torch.randn(N, device=dev)
    y = _ext.gemm_fwd(x, w, b, tile=tile)
    _check(y, x.float() @ w.float().t() + b)
    y0 = _ext.gemm_fwd(x, w, None, tile=tile)
    _check(y0, x.float() @ w.float().t())


@pytest.mark.parametrize("M,N,K", [(1000, 512, 192), (2100, 1024, 256), (320, 3072, 768)])
@pytest.mark.parametrize("tile", [256, 128, 64, 32])
def test_forward_bias_gelu(dev, M, N, K, tile):
    from bridgeqa_amd import _ext
    x, w = _rand((M, K), dev, 3), _rand((N, K), dev, 4, 0.1)
    b = torch.randn(N, device=dev)
    y, act = _ext.gemm_fwd(x, w, b, gelu=True, tile=tile)
    ref = x.float() @ w.float().t() + b
    _check(y, ref)
    _check(act, _gelu(y.float()))          # the activation is taken at the SAVED (bf16) pre-activation
    _check(act, _gelu(ref))


def test_identity_asymmetric(dev):
    """P = I with an asymmetric Q catches a transposed or permuted output map (integer data: exact)"""
    from bridgeqa_amd import _ext
    N = 256
    w = torch.eye(N, device=dev, dtype=torch.bfloat16)
    x = (torch.arange(512 * N, device=dev).reshape(512, N) % 251).to(torch.bfloat16)
    for tile in (256, 128, 64, 32):
        y = _ext.gemm_fwd(x, w, None, tile=tile)
        assert torch.equal(y, x), tile
        dx = _ext.gemm_dx(x, w, tile=tile)
        assert torch.equal(dx, x), tile
    dw = _ext.gemm_dw(torch.eye(512, device=dev, dtype=torch.bfloat16)[:, :256].contiguous(), x[:512], tile=256)
    assert torch.equal(dw, x[:256].float())


@pytest.mark.parametrize("M,N,K", [(1000, 384, 512), (1500, 768, 256), (16400, 768, 768), (320, 768, 3072), (80, 1536, 768)])
@pytest.mark.parametrize("tile", [256, 128, 64, 32])
def test_dx(dev, M, N, K, tile):
    """dx = dy @ W (contraction over N): P = W contraction-major (transposed LDS reads)"""
    from bridgeqa_amd import _ext
    if tile < 128 and M * K > 4e6:
        pytest.skip("small-tile kernels are for small problems")
    dy, w = _rand((M, N), dev, 5), _rand((N, K), dev, 6, 0.1)
    dx = _ext.gemm_dx(dy, w, tile=tile)
    _check(dx, dy.float() @ w.float())


@pytest.mark.parametrize("M,N,K", [(1000, 384, 512), (2000, 768, 3072), (320, 768, 3072)])
@pytest.mark.parametrize("tile", [256, 64, 32])
def test_dx_dgelu_colsum(dev, M, N, K, tile):
    """the fc2 input gradient with the GELU derivative and fc1's bias gradient fused in"""
    from bridgeqa_amd import _ext
    dy, w = _rand((M, N), dev, 7), _rand((N, K), dev, 8, 0.1)
    pre = _rand((M, K), dev, 9, 1.5)
    cs = torch.zeros(K, device=dev)
    dx = _ext.gemm_dx(dy, w, pre_act=pre, colsum=cs, tile=tile)
    p32 = pre.float().requires_grad_(True)
    _gelu(p32).backward(dy.float() @ w.float())
    _check(dx, p32.grad)
    ref_cs = dx.float().sum(0)
    assert ((cs - ref_cs).abs().max() / (ref_cs.abs().max() + 1e-20)).item() < 1e-4


@pytest.mark.parametrize("M,N,K", [(1000, 512, 768), (1024, 256, 256), (16400, 768, 768), (320, 3072, 768), (80, 768, 768), (20, 768, 1536)])
@pytest.mark.parametrize("tile", [256, 128, 64])
def test_dw(dev, M, N, K, tile):
    """dw = dy^T @ x (contraction over the M rows, any M: the ragged last K tile is zero-filled by the bounds-checked
    LDS-DMA), fp32 out"""
    from bridgeqa_amd import _ext
    if tile == 128 and M < 128:
        pytest.skip("the persistent 256 x 128 kernel needs two K tiles")
    dy, x = _rand((M, N), dev, 10), _rand((M, K), dev, 11)
    dw = _ext.gemm_dw(dy, x, tile=tile)
    _check(dw, dy.float().t() @ x.float(), f32=True)


@pytest.mark.parametrize("M,N,K", [(1000, 384, 512), (2000, 768, 3072), (16400, 768, 3072), (130, 768, 256)])
def test_dx_epilogues_on_the_256x128_tile(dev, M, N, K):
    """csrc/gemm_mid.hip (tile=128: 256 x 128 tiles, persistent, two workgroups per CU): the input-gradient form, plain,
    with a second gradient added and with the GELU derivative in the epilogue; ragged last row tiles
    (1000 = 7 x 128 + 104, 16400 = 128 x 128 + 16, 130 = 128 + 2)"""
    from bridgeqa_amd import _ext
    dy, w = _rand((M, N), dev, 7), _rand((N, K), dev, 8, 0.1)
    pre = _rand((M, K), dev, 9, 1.5)
    other = _rand((M, K), dev, 12)
    _check(_ext.gemm_dx(dy, w, add=other, tile=128), dy.float() @ w.float() + other.float())
    _check(_ext.gemm_dx(dy, w, tile=128), dy.float() @ w.float())
    dx = _ext.gemm_dx(dy, w, pre_act=pre, tile=128)   # gelu' evaluated in the epilogue (no LDS table on this tile)
    p32 = pre.float().requires_grad_(True)
    _gelu(p32).backward(dy.float() @ w.float())
    _check(dx, p32.grad)
    with pytest.raises(RuntimeError):   # no column sums on this tile: rejected, never silently dropped
        _ext.gemm_dx(dy, w, colsum=torch.zeros(K, device=dev), tile=128)


def test_256x128_tile_grouped_ragged_and_repeatable_under_load(dev):
    """tile=128: a grouped launch of problems with ragged i and j extents (Ni not a multiple of 256, Nj not of 128), and
    -- single-buffered P units restaged one phase after their last read, counted waits across barriers -- bitwise
    repeatability of the c3 shapes while another stream keeps the memory system busy (a mis-placed wait shows up as rare
    wrong tiles)"""
    from bridgeqa_amd import _ext
    probs, refs = [], []
    for k, (M, N, K) in enumerate([(1000, 264, 192), (129, 768, 768), (4416, 1536, 768), (70, 8, 128), (16720, 1536, 768)]):
        x, w = _rand((M, K), dev, 20 + k), _rand((N, K), dev, 40 + k, 0.1)
        b = torch.randn(N, device=dev)
        probs.append(dict(P=w, Q=x, out=torch.empty(M, N, device=dev, dtype=torch.bfloat16), bias=b))
        refs.append(x.float() @ w.float().t() + b)
    _ext.gemm_grouped(probs, 0, _ext.EPI_BIAS, 128)
    for p, r in zip(probs, refs):
        _check(p["out"], r)
    M = 16400
    x, w, dy = _rand((M, 768), dev, 50), _rand((2304, 768), dev, 51, 0.05), _rand((M, 2304), dev, 52)
    w2, h = _rand((768, 3072), dev, 53, 0.05), _rand((M, 3072), dev, 54)
    dy2 = _rand((M, 768), dev, 55)
    y0 = _ext.gemm_fwd(x, w, None, tile=128)
    dx0 = _ext.gemm_dx(dy, w, tile=128)
    g0 = _ext.gemm_dx(dy2, w2, add=h, tile=128)
    g1 = _ext.gemm_dx(dy2, w2, pre_act=h, tile=128)
    _check(y0, x.float() @ w.float().t())
    _check(dx0, dy.float() @ w.float())
    side = torch.cuda.Stream()
    big = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    for it in range(12):
        with torch.cuda.stream(side):
            for _ in range(4):
                big.add_(1)     # HBM-bound traffic beside the GEMMs
        assert torch.equal(_ext.gemm_fwd(x, w, None, tile=128), y0), it
        assert torch.equal(_ext.gemm_dx(dy, w, tile=128), dx0), it
        assert torch.equal(_ext.gemm_dx(dy2, w2, add=h, tile=128), g0), it
        assert torch.equal(_ext.gemm_dx(dy2, w2, pre_act=h, tile=128), g1), it
    torch.cuda.synchronize()


def test_dw_with_bias_gradient_from_the_same_launch(dev):
    """the weight-gradient form of the 256-tile / 256 x 128-tile kernels with colsum set: colsum[j] = sum over the contraction of Q (= the bias
    gradient, column sums of dY), from all-ones MFMAs in the i = 0 tiles; grouped problems of ragged sizes (rows not a
    multiple of 64, out features not a multiple of 256, several i tiles) -- and dW itself unchanged by it"""
    from bridgeqa_amd import _ext
    flags = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
    probs, dys = [], []
    for k, (M, N, K) in enumerate([(1000, 768, 768), (16400, 2304, 768), (1025, 776, 3072), (4416, 1536, 768), (130, 8, 64)]):
        dy, x = _rand((M, N), dev, 60 + k), _rand((M, K), dev, 80 + k)
        probs.append(dict(P=x, Q=dy, out=torch.empty(N, K, device=dev), colsum=torch.full((N,), float("nan"), device=dev)))
        dys.append(dy)
    for tile in (256, 128, 64):
        for p in probs:
            p["colsum"].fill_(float("nan"))
        _ext.gemm_grouped(probs, flags, _ext.EPI_NONE, tile)
        plain = [dict(P=p["P"], Q=p["Q"], out=torch.empty_like(p["out"])) for p in probs]
        _ext.gemm_grouped(plain, flags, _ext.EPI_NONE, tile)
        for p, q, dy in zip(probs, plain, dys):
            assert torch.equal(p["out"], q["out"])
            ref = dy.float().sum(0)
            assert torch.isfinite(p["colsum"]).all()
            assert ((p["colsum"] - ref).abs().max() / (ref.abs().max() + 1e-20)).item() < 1e-5
    # split contraction (64-tile kernel, ksplit pieces): out and colsum accumulate with atomics onto zeros
    dy, x = dys[1], probs[1]["P"]
    out, cs = torch.zeros(dy.shape[1], x.shape[1], device=dev), torch.zeros(dy.shape[1], device=dev)
    _ext.gemm_grouped([dict(P=x, Q=dy, out=out, colsum=cs, ksplit=7)], flags, _ext.EPI_NONE, 64)
    ref = dy.float().sum(0)
    assert ((cs - ref).abs().max() / ref.abs().max()).item() < 1e-5
    _check(out, dy.float().t() @ x.float(), f32=True)


@pytest.mark.parametrize("R,N,K", [(70000, 64, 136), (33000, 128, 64), (9000, 256, 128), (5000, 128, 264)])
@pytest.mark.parametrize("ksplit", [8, 48, 5, 1])
def test_dw_cut_contraction_detector_shapes(dev, R, N, K, ksplit):
    """the detector's weight gradients: a contraction over very many rows cut into ksplit pieces that accumulate with
    atomics onto zeros; ksplit % 8 == 0 takes the XCD-aware slot order (tiles of one piece on one XCD), other values the
    piece-major order -- every (tile, piece) pair must be computed exactly once.  Two problems in one launch: the second
    starts at a tile offset that is not a multiple of 8."""
    from bridgeqa_amd import _ext
    flags = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
    dy, x = _rand((R, N), dev, 30), _rand((R, K), dev, 31)
    dy2, x2 = _rand((777, 64), dev, 32), _rand((777, 72), dev, 33)
    out, out2 = torch.zeros(N, K, device=dev), torch.zeros(64, 72, device=dev)
    _ext.gemm_grouped([dict(P=x2, Q=dy2, out=out2, ksplit=3), dict(P=x, Q=dy, out=out, ksplit=ksplit)], flags,
                      _ext.EPI_NONE, 64)
    _check(out, dy.float().t() @ x.float(), f32=True)
    _check(out2, dy2.float().t() @ x2.float(), f32=True)
    out.zero_()
    _ext.gemm_grouped([dict(P=x, Q=dy, out=out, ksplit=ksplit)], flags, _ext.EPI_NONE, 64)
    _check(out, dy.float().t() @ x.float(), f32=True)


@pytest.mark.parametrize("R,N,K", [(70001, 64, 136), (33000, 128, 64), (9000, 256, 120), (5000, 64, 64), (4100, 128, 136),
                                   (3000, 128, 128), (2500, 256, 64), (2000, 64, 248), (1500, 128, 200), (64, 64, 72),
                                   (130, 128, 192), (5000, 128, 264), (3000, 256, 136)])
@pytest.mark.parametrize("wgs", [0, 7])
def test_wgrad_rows(dev, R, N, K, wgs):
    """bq_wgrad_rows_bf16 (whole rows staged, all output tiles of a row piece in one workgroup, slices summed by a second
    kernel) = dy^T x; every supported (input, output) unit combination, row counts that are not multiples of 64, an input
    row stride larger than its channel count (zero padding columns), more workgroups than K tiles"""
    from bridgeqa_amd import _ext
    assert _ext.wgrad_rows_ok(K, N)
    dy = _rand((R, N), dev, 40)
    ld = K + 8
    xbuf = torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)
    xbuf[:, :K] = _rand((R, K), dev, 41)
    x = xbuf[:, :K]
    out = torch.full((N, ld), float("nan"), device=dev)
    _ext.wgrad_rows(torch.as_strided(xbuf, (R, ld), (ld, 1)), dy, out, wgs)       # whole padded rows as channels
    ref = dy.float().t() @ xbuf.float()
    _check(out, ref, f32=True)
    out2 = torch.full((N, K), float("nan"), device=dev)
    _ext.wgrad_rows(x, dy, out2, wgs)                               # a column view: stride ld, K channels
    _check(out2, ref[:, :K], f32=True)
    out3 = torch.full((N, ld), float("nan"), device=dev)
    _ext.wgrad_rows(x, dy, out3, wgs)                               # K channels into a wider buffer: padding zeroed
    assert torch.equal(out3[:, :K], out2) and (out3[:, K:] == 0).all()
    again = torch.empty_like(out2)
    _ext.wgrad_rows(x, dy, again, wgs)
    assert torch.equal(again, out2)                                 # fixed summation order: bitwise reproducible


def test_wgrad_rows_rejects_unsupported_shapes(dev):
    from bridgeqa_amd import _ext
    assert not _ext.wgrad_rows_ok(328, 128) and not _ext.wgrad_rows_ok(64, 192) and not _ext.wgrad_rows_ok(256, 256)
    assert not _ext.wgrad_rows_ok(320, 64)
    x, dy = _rand((100, 328), dev, 1), _rand((100, 128), dev, 2)
    with pytest.raises(RuntimeError):
        _ext.wgrad_rows(x, dy, torch.zeros(128, 328, device=dev))


def test_grouped_launch(dev):
    """several problems of different sizes in ONE launch (the deferred weight gradients of a layer stack)"""
    from bridgeqa_amd import _ext
    probs, refs = [], []
    for k, (M, N, K) in enumerate([(700, 768, 768), (1000, 2304, 768), (512, 768, 3072), (999, 3072, 768)] * 3):
        dy, x = _rand((M, N), dev, 20 + k), _rand((M, K), dev, 40 + k)
        out = torch.empty(N, K, device=dev)
        probs.append(dict(P=x, Q=dy, out=out))
        refs.append(dy.float().t() @ x.float())
    for tile in (256, 64):
        for p in probs:
            p["out"].fill_(float("nan"))
        _ext.gemm_grouped(probs, _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32, _ext.EPI_NONE, tile)
        for p, r in zip(probs, refs):
            _check(p["out"], r, f32=True)
    # more problems than one launch holds
    many = []
    for k in range(_ext._lib.bq_gemm_max_problems() + 5):
        x, w = _rand((90, 128), dev, 100 + k), _rand((64, 128), dev, 200 + k)
        many.append(dict(P=w, Q=x, out=torch.empty(90, 64, device=dev, dtype=torch.bfloat16)))
    _ext.gemm_grouped(many, 0, _ext.EPI_NONE, 32)
    for p in many:
        _check(p["out"], p["Q"].float() @ p["P"].float().t())


def test_strided_operands(dev):
    """operands that are column slices of wider tensors (a fused QKV output, a slice of a hoisted projection)"""
    from bridgeqa_amd import _ext
    big = _rand((1100, 2304), dev, 60)
    x = big[:, 768:1536]
    w = _rand((768, 768), dev, 61, 0.1)
    outbig = torch.zeros(1100, 1536, device=dev, dtype=torch.bfloat16)
    out = outbig[:, 768:]
    _ext.gemm_grouped([dict(P=w, Q=x, out=out)], 0, _ext.EPI_NONE, 256)
    _check(out, x.float() @ w.float().t())
    assert outbig[:, :768].abs().max().item() == 0


def test_repeatable_under_load(dev):
    """The K loop keeps LDS-DMA stages in flight across barriers: a mis-placed wait shows up as rare wrong tiles.
    Same inputs, many launches back to back (a warm and a cold L2), every output bit-identical to the first and equal
    to the reference."""
    from bridgeqa_amd import _ext
    x, w = _rand((16400, 768), dev, 70), _rand((3072, 768), dev, 71, 0.1)
    dy = _rand((16400, 3072), dev, 72)
    ref = x.float() @ w.float().t()
    y0 = _ext.gemm_fwd(x, w, None, tile=256)
    _check(y0, ref)
    dx0 = _ext.gemm_dx(dy, w, tile=256)
    _check(dx0, dy.float() @ w.float())
    dw0 = _ext.gemm_dw(dy, x, tile=256)
    _check(dw0, dy.float().t() @ x.float(), f32=True)
    junk = torch.empty(1 << 28, device=dev, dtype=torch.uint8)
    side = torch.cuda.Stream()
    big = torch.zeros(256 << 20, device=dev, dtype=torch.uint8)
    side.wait_stream(torch.cuda.current_stream())
    big.record_stream(side)
    try:
        for it in range(12):
            if it % 3 == 0:
                junk.fill_(it)  # evict L2 / Infinity Cache
            with torch.cuda.stream(side):
                for _ in range(4):
                    big.add_(1)     # HBM-bound traffic beside the GEMMs
            assert torch.equal(_ext.gemm_fwd(x, w, None, tile=256), y0), it
            assert torch.equal(_ext.gemm_dx(dy, w, tile=256), dx0), it
            assert torch.equal(_ext.gemm_dw(dy, x, tile=256), dw0), it
    finally:
        torch.cuda.synchronize()   # (no side-stream write outlives the test, also when an assert ends it)


def test_rejects_bad_arguments(dev):
    from bridgeqa_amd import _ext
    x, w = _rand((64, 100), dev, 80), _rand((64, 100), dev, 81)
    with pytest.raises(RuntimeError):
        _ext.gemm_fwd(x, w)                       # K-contiguous operands need K % 64 == 0 (and ld % 8 == 0)
    with pytest.raises(RuntimeError):
        _ext.gemm_fwd(x.cpu(), w.cpu())           # no CPU path


def test_lm_head_cross_entropy_vs_torch(dev):
    """fusion_ops.lm_loss on the kernels (cross-entropy epilogue of the GEMM + csrc/lmhead.hip) at the real head size
    (vocabulary 30524 -- not a multiple of anything convenient --, hidden 768, 32 x 5 rows) and at a tiny one, against
    torch's fp32 composition of the reference (med.py:1417-1432): per-sequence loss 2e-3 relative (operands bf16, loss
    statistics fp32), gradients of the hidden states / the tied weight / the bias rel-L2 2e-2."""
    from bridgeqa_amd import fusion_ops as ops
    prev = ops.set_compute_dtype(torch.bfloat16)
    try:
        for (B, L, D, V) in ((32, 5, 768, 30524), (3, 6, 256, 200)):
            g = torch.Generator().manual_seed(V)
            w = torch.nn.Parameter((torch.randn(V, D, generator=g) * 0.05).to(dev))
            b = torch.nn.Parameter((torch.randn(V, generator=g) * 0.1).to(dev))
            h0 = torch.randn(B, L, D, generator=g).to(dev).to(torch.bfloat16)
            labels = torch.randint(0, V, (B, L), generator=g).to(dev)
            labels[0, 2:] = -100
            labels[:, 0] = -100
            wseq = torch.rand(B, generator=g).to(dev) + 0.5
            h = h0.clone().requires_grad_(True)
            logits, loss = ops.lm_loss(h, w, b, labels, label_smoothing=0.1)
            assert logits.shape == (B, L, V) and logits.dtype == torch.bfloat16
            logits_copy = logits.float().clone()
            (loss * wseq).sum().backward()
            hr = h0.float().clone().requires_grad_(True)
            wr = w.detach().to(torch.bfloat16).float().requires_grad_(True)
            br = b.detach().clone().requires_grad_(True)
            lr = hr @ wr.t() + br
            ce = torch.nn.functional.cross_entropy(lr[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), reduction="none",
                                                   label_smoothing=0.1).view(B, -1).sum(1)
            (ce * wseq).sum().backward()
            rel = lambda x, y: ((x.float() - y.float()).norm() / (y.float().norm() + 1e-20)).item()
            assert rel(logits_copy, lr) < 3e-3
            assert (loss - ce).abs().max().item() <= 2e-3 * ce.abs().max().item(), (loss, ce)
            assert rel(h.grad, hr.grad) < 2e-2, rel(h.grad, hr.grad)
            assert rel(w.grad, wr.grad) < 2e-2, rel(w.grad, wr.grad)
            assert rel(b.grad, br.grad) < 2e-2, rel(b.grad, br.grad)
    finally:
        ops.set_compute_dtype(prev)


@pytest.mark.parametrize("M,N,K", [(640, 768, 3072), (160, 768, 3072), (200, 264, 1600), (320, 768, 2304), (77, 128, 1536 + 64)])
@pytest.mark.parametrize("tile", [64, 32])
def test_long_contraction_two_k_tiles_per_step(dev, M, N, K, tile):
    """the small-tile kernels' KT = 2 instantiation (two K tiles per pipeline step, chosen by the launcher when every
    contraction of a small launch has >= 24 K tiles): forward with bias, forward without, and the input-gradient form;
    odd K-tile counts (1600 = 25 tiles, 1600 = 1536 + 64) exercise the zero-staged half step at the end"""
    from bridgeqa_amd import _ext
    x, w = _rand((M, K), dev, 21), _rand((N, K), dev, 22, 0.05)
    b = torch.randn(N, device=dev)
    _check(_ext.gemm_fwd(x, w, b, tile=tile), x.float() @ w.float().t() + b)
    _check(_ext.gemm_fwd(x, w, None, tile=tile), x.float() @ w.float().t())
    # dX = dY W with the contraction over N: a long one needs a wide layer
    dy, w2 = _rand((M, K), dev, 23), _rand((K, N), dev, 24, 0.05)      # dY (M, K_out = K), W (K_out, N_in = N)
    _check(_ext.gemm_dx(dy, w2, tile=tile), dy.float() @ w2.float())


@pytest.mark.parametrize("R,K,N", [(16384, 256, 259), (4096, 128, 97), (100, 128, 97), (1000, 64, 8)])
def test_rows_linear_f32_odd_output_widths(dev, R, K, N):
    """pytorch_utils.rows_linear_f32 (the detector's 259- / 97-channel output layers, voting_module.py:27-31 /
    proposal_module.py:48-56, on the MFMA GEMM family with fp32 results) against F.linear on the same bf16-rounded
    operands: output, input gradient, weight and bias gradients"""
    from bridgeqa_amd import pytorch_utils as pt
    torch.manual_seed(0)
    rows = _rand((R, K), dev, 70).requires_grad_(True)
    w = (torch.randn(N, K, device=dev) * 0.1).requires_grad_(True)
    b = torch.randn(N, device=dev).requires_grad_(True)
    gy = torch.randn(R, N, device=dev)
    y = pt.rows_linear_f32(rows, w, b)
    assert y.dtype == torch.float32 and y.shape == (R, N)
    y.backward(gy)
    r32 = rows.detach().float().requires_grad_(True)
    w32 = w.detach().to(torch.bfloat16).float().requires_grad_(True)
    b32 = b.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.linear(r32, w32, b32)
    ref.backward(gy.to(torch.bfloat16).float())
    rel = lambda a, c: ((a.float() - c).norm() / (c.norm() + 1e-20)).item()
    assert rel(y, ref) < 1e-5
    assert rel(rows.grad, r32.grad) < 4e-3          # bf16 result
    assert rel(w.grad, w32.grad) < 1e-4 and rel(b.grad, b32.grad) < 1e-4


def test_background_launch_equals_the_full_grid(dev):
    """BQ_GEMM_BACKGROUND (one persistent workgroup per CU for a side-stream GEMM, include/bqhip_fusion.h): same tiles, same
    order of accumulation -- bit-equal results for the forward, the ADD-epilogue dX and the weight-gradient forms; the flag is
    refused for tiles that have no persistent grid"""
    from bridgeqa_amd import _ext
    x, w, b = _rand((16400, 768), dev, 90), _rand((1536, 768), dev, 91, 0.05), torch.randn(1536, device=dev)
    assert torch.equal(_ext.gemm_fwd(x, w, b, background=True), _ext.gemm_fwd(x, w, b))
    dy, add = _rand((16400, 1536), dev, 92), _rand((16400, 768), dev, 93)
    assert torch.equal(_ext.gemm_dx(dy, w, add=add, background=True), _ext.gemm_dx(dy, w, add=add))
    flags = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
    o1, o2 = torch.empty(1536, 768, device=dev), torch.empty(1536, 768, device=dev)
    _ext.gemm_grouped([dict(P=x, Q=dy, out=o1)], flags | _ext.GEMM_BACKGROUND, _ext.EPI_NONE, 128)
    _ext.gemm_grouped([dict(P=x, Q=dy, out=o2)], flags, _ext.EPI_NONE, 128)
    assert torch.equal(o1, o2)
    import ctypes
    d = (_ext._GemmDesc * 1)()
    d[0].P, d[0].Q, d[0].out = x.data_ptr(), dy.data_ptr(), o1.data_ptr()
    d[0].ldp, d[0].ldq, d[0].ldo, d[0].Ni, d[0].Nj, d[0].Kc = 768, 1536, 768, 768, 1536, 16400
    assert _ext._lib.bq_gemm_bf16(d, 1, flags | _ext.GEMM_BACKGROUND, _ext.EPI_NONE, 256, None) != 0


# ---- batched-row maps (bq_gemm_desc q_rpb / o_rpb, ABI 2): a (batch, rows, cols) view with a batch stride as the row
# operand or the output -- what replaced torch.cat in front of the twin encoder's K/V projections (med.py:549-562) -----
MAP_CASES = [(16, 1025, 20, 768, 1536), (3, 130, 7, 256, 512), (2, 64, 64, 128, 256), (5, 20, 300, 192, 320)]


@pytest.mark.parametrize("B,R1,R2,K,N", MAP_CASES)
@pytest.mark.parametrize("tile", [128, 64, 32])
def test_forward_writes_row_ranges_of_one_output(dev, B, R1, R2, K, N, tile):
    """two row sources (B, R1, K) and (B, R2, K) through the same weights into ONE (B, R1 + R2, N) tensor: each problem's
    output rows are a batched-row view of it; equals the projection of the concatenation"""
    from bridgeqa_amd import _ext
    if tile < 128 and B * R1 * N > 4e6:
        pytest.skip("small-tile kernels are for small problems")
    xa, xb, w = _rand((B, R1, K), dev, 21), _rand((B, R2, K), dev, 22), _rand((N, K), dev, 23, 0.1)
    b = torch.randn(N, device=dev)
    out = torch.full((B, R1 + R2, N), float("nan"), device=dev, dtype=torch.bfloat16)
    _ext.gemm_grouped([dict(P=w, Q=xa.view(B * R1, K), out=out[:, :R1], bias=b),
                       dict(P=w, Q=xb.view(B * R2, K), out=out[:, R1:], bias=b)], 0, _ext.EPI_BIAS, tile)
    ref = torch.cat((xa, xb), 1).float() @ w.float().t() + b
    _check(out, ref)


@pytest.mark.parametrize("B,R1,R2,K,N", MAP_CASES)
@pytest.mark.parametrize("tile", [128, 64, 32])
def test_dx_reads_row_ranges_and_accumulates_in_place(dev, B, R1, R2, K, N, tile):
    """input gradient of the same: Q = the row range of the (B, R1 + R2, N) gradient read in place (q map); the first
    source's dX is ADDED into an existing buffer (EPI_ADD, aux = out), the second's to a tapped gradient"""
    from bridgeqa_amd import _ext
    if tile < 128 and B * R1 * N > 4e6:
        pytest.skip("small-tile kernels are for small problems")
    g, w = _rand((B, R1 + R2, N), dev, 31), _rand((N, K), dev, 32, 0.1)
    acc0, tapg = _rand((B * R1, K), dev, 33), _rand((B * R2, K), dev, 34)
    acc = acc0.clone()
    dxb = torch.empty(B * R2, K, device=dev, dtype=torch.bfloat16)
    _ext.gemm_grouped([dict(P=w, Q=g[:, :R1], out=acc, aux=acc), dict(P=w, Q=g[:, R1:], out=dxb, aux=tapg)],
                      _ext.GEMM_P_XC, _ext.EPI_ADD, tile)
    _check(acc, g[:, :R1].reshape(-1, N).float() @ w.float() + acc0.float())
    _check(dxb, g[:, R1:].reshape(-1, N).float() @ w.float() + tapg.float())
    # a mapped OUTPUT with a second operand laid out like it (aux under the same map)
    base = _rand((B, R1 + R2, K), dev, 35)
    out = base.clone()
    x = _rand((B * R1, N), dev, 36)
    _ext.gemm_grouped([dict(P=w, Q=x, out=out[:, :R1], aux=out[:, :R1])], _ext.GEMM_P_XC, _ext.EPI_ADD, tile)
    _check(out[:, :R1], (x.float() @ w.float()).view(B, R1, K) + base[:, :R1].float())
    assert torch.equal(out[:, R1:], base[:, R1:])                       # the other row range is untouched


@pytest.mark.parametrize("B,R1,R2,K,N", MAP_CASES)
def test_dw_from_two_row_sources(dev, B, R1, R2, K, N):
    """weight gradient over the rows of BOTH sources: the first stored by the tile its size picks (256: the contraction-row
    map walks the batches incrementally; 64: one division per DMA), the second ADDED by the small-tile kernel's atomic
    epilogue (accum), column sums (bias gradient) likewise"""
    from bridgeqa_amd import _ext
    g = _rand((B, R1 + R2, N), dev, 41)
    xa, xb = _rand((B * R1, K), dev, 42), _rand((B * R2, K), dev, 43)
    f = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
    ref = g[:, :R1].reshape(-1, N).float().t() @ xa.float() + g[:, R1:].reshape(-1, N).float().t() @ xb.float()
    refb = g.float().sum((0, 1))
    for tile in ([256, 64] if R1 >= 64 else [64]):
        dw = torch.empty(N, K, device=dev)
        db = torch.empty(N, device=dev)
        _ext.gemm_grouped([dict(P=xa, Q=g[:, :R1], out=dw, colsum=db)], f, _ext.EPI_NONE, tile)
        _ext.gemm_grouped([dict(P=xb, Q=g[:, R1:], out=dw, colsum=db, accum=True)], f, _ext.EPI_NONE, 64)
        _check(dw, ref, f32=True)
        _check(db, refb, f32=True)


def test_row_maps_reject_what_the_kernels_cannot_address(dev):
    from bridgeqa_amd import _ext
    w, x = _rand((256, 128), dev, 51), _rand((4, 100, 128), dev, 52)
    out = torch.empty(4, 120, 256, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):     # tile 256 maps only the contraction rows of its weight-gradient form
        _ext.gemm_grouped([dict(P=w, Q=x.view(400, 128), out=out[:, :100])], 0, _ext.EPI_NONE, 256)
    dw = torch.empty(256, 128, device=dev)
    with pytest.raises(RuntimeError):     # accum needs the small-tile kernel
        _ext.gemm_grouped([dict(P=x.view(400, 128), Q=_rand((400, 256), dev, 53), out=dw, accum=True)],
                          _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32, _ext.EPI_NONE, 256)


@pytest.mark.parametrize("M,N,K", [(640, 768, 768), (640, 2304, 768), (640, 3072, 768), (640, 768, 3072), (80, 1536, 768),
                                   (16400, 768, 768)])
@pytest.mark.parametrize("epi", ["none", "add", "dgelu"])
def test_dx_on_a_transposed_weight_equals_the_contraction_major_read(dev, M, N, K, epi):
    """the text side's input gradients read a K-contiguous copy W^T of the weight (csrc/transpose.hip,
    fusion_state.transposed_shadow): same products in the same order as the contraction-major read of W -- identical bits"""
    from bridgeqa_amd import _ext
    dy, w = _rand((M, N), dev, 51), _rand((N, K), dev, 52, 0.1)
    aux = _rand((M, K), dev, 53, 1.5) if epi != "none" else None
    kw = {"add": aux} if epi == "add" else ({"pre_act": aux} if epi == "dgelu" else {})
    a = _ext.gemm_dx(dy, w, **kw)
    b = _ext.gemm_dx(dy, w, wt=w.t().contiguous(), **kw)
    assert torch.equal(a, b)
    ref = dy.float() @ w.float()
    if epi == "add":
        ref = ref + aux.float()
    elif epi == "dgelu":
        p32 = aux.float().requires_grad_(True)
        _gelu(p32).backward(ref)
        ref = p32.grad
    _check(b, ref)


def test_multi_tensor_transpose(dev):
    """bq_transpose_multi_bf16: every registered (N, K) operand -> its (K, N) copy in one launch, row blocks of a
    concatenated buffer (a strided source) included"""
    from bridgeqa_amd import _ext
    cat = _rand((2304, 768), dev, 61)
    srcs = [_rand((768, 768), dev, 62), cat[768:2304], _rand((3072, 768), dev, 63), _rand((768, 3072), dev, 64),
            _rand((64, 128), dev, 65), _rand((1536, 832), dev, 66)[:, :768]]
    dsts = [torch.zeros(s.shape[1], s.shape[0], dtype=torch.bfloat16, device=dev) for s in srcs]
    table, chunks = _ext.transpose_table(list(zip(srcs, dsts)), dev)
    assert chunks.shape[0] == sum(s.shape[0] // 64 * (s.shape[1] // 64) for s in srcs)
    for max_wgs in (0, 7, 100000):   # one workgroup per tile; a small grid walking the tiles; a limit above the tile count
        for d in dsts:
            d.zero_()
        _ext.transpose_multi(table, chunks, max_wgs)
        for s, d in zip(srcs, dsts):
            assert torch.equal(d, s.t())
    with pytest.raises(RuntimeError):
        _ext.transpose_table([(_rand((100, 128), dev, 67), torch.zeros(128, 100, dtype=torch.bfloat16, device=dev))], dev)


def _sk_forms(form, on):
    """form 128: the 256 x 128 kernel's stream-K (csrc/gemm_mid.hip), form 256: the 256 x 256 kernel's (csrc/gemm.hip); the
    other form off while one is tested; (None, ..): the product defaults"""
    from bridgeqa_amd import _ext
    if form is None:
        _ext.streamk_enable(False)
        _ext.streamk256_enable(False)
    else:
        _ext.streamk_enable(on and form == 128)
        _ext.streamk256_enable(on and form == 256)


@pytest.mark.parametrize("form", [128, 256])
@pytest.mark.parametrize("M,N,K", [(16400, 768, 3072), (16384, 768, 3072), (16400, 768, 1536), (9000, 1024, 2048),
                                   (16720, 768, 3072)])
def test_stream_k_equals_whole_tiles(dev, M, N, K, form):
    """the stream-K forms of the 256 x 128 kernel (csrc/gemm_mid.hip header: a tile cut across workgroups, finished by the
    last arriver through fp32 slabs) and of the 256 x 256 kernel (csrc/gemm.hip: the same protocol around that kernel's
    per-segment pipeline) on the ViT MLP's long-contraction launches --
    forward + bias, dX on the transposed weight copy with and without the ADD epilogue -- against torch fp32 and against the
    same launches on whole tiles (different fp32 summation order: equal up to one bf16 rounding on a few elements), five
    times over (tickets must come back to zero), ragged row blocks included"""
    from bridgeqa_amd import _ext
    x, w = _rand((M, K), dev, 71), _rand((N, K), dev, 72, 0.05)
    b = torch.randn(N, device=dev)
    ref = x.float() @ w.float().t() + b
    _sk_forms(form, False)
    whole = _ext.gemm_fwd(x, w, b, tile=128)
    _sk_forms(form, True)
    outs = [_ext.gemm_fwd(x, w, b, tile=128) for _ in range(5)]
    torch.cuda.synchronize()
    for y in outs:
        _check(y, ref)
        assert torch.equal(y, outs[0])                    # same cuts, same order of additions: reproducible
        assert ((y.float() - whole.float()).abs() > 0).float().mean().item() < 0.05
        assert ((y.float() - whole.float()).abs().max() / ref.abs().max()).item() < 1e-2
    # dX of the same layer shape: dy (M, K_out = N) through W (N, K) read as W^T K-contiguous
    dy, w2 = _rand((M, K), dev, 73), _rand((K, N), dev, 74, 0.05)      # contraction K, out features N
    aux = _rand((M, N), dev, 75)
    wt = w2.t().contiguous()
    for add in (None, aux):
        got = [_ext.gemm_dx(dy, w2, add=add, wt=wt, tile=128) for _ in range(3)]
        r = dy.float() @ w2.float() + (add.float() if add is not None else 0.0)
        torch.cuda.synchronize()
        for g in got:
            _check(g, r)
            assert torch.equal(g, got[0])
    _sk_forms(None, None)


@pytest.mark.parametrize("form", [128, 256])
def test_stream_k_under_load_and_graph_replay(dev, form):
    """the hand-off protocol with the chip busy (a second stream keeps launching bandwidth-bound kernels, so workgroups of
    one launch are not all resident at once and arrive in every order) and replayed from a HIP graph"""
    from bridgeqa_amd import _ext
    _sk_forms(form, True)
    M, N, K = 16400, 768, 3072
    x, w = _rand((M, K), dev, 81), _rand((N, K), dev, 82, 0.05)
    b = torch.randn(N, device=dev)
    ref = x.float() @ w.float().t() + b
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    junk = torch.empty(64 << 20, device=dev)
    want = _ext.gemm_fwd(x, w, b, tile=128)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        _ext.gemm_fwd(x, w, b, tile=128)                 # (registers the stream's workspace outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s1):
        y = _ext.gemm_fwd(x, w, b, tile=128)
    for it in range(6):
        with torch.cuda.stream(s2):
            for _ in range(8):
                junk.mul_(1.0001)
        with torch.cuda.stream(s1):
            g.replay()
        torch.cuda.synchronize()
        _check(y, ref)
        # (the workgroup that arrives LAST folds a cut tile, its own accumulators first: under load the arrival order -- and
        # with it the order of the fp32 additions -- varies, so replays agree to the last bf16 bit on all but a few elements;
        # one full-suite run in round 6 saw a differing element at the sixth replay, six stand-alone runs none)
        diff = (y.float() - want.float()).abs()
        assert (diff > 0).float().mean().item() < 1e-3 and (diff.max() / ref.abs().max()).item() < 1e-2, it
    _sk_forms(None, None)
