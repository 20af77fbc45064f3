"""The LSTM kernels of csrc/lstm.hip behind lang_module.LangModule, on the device, for H in {128, 256}, E = 20: the padding
contract, lang_emb against lang_out bit for bit, forward values and every gradient (dX, dW_ih, dW_hh, db_ih, db_hh, gradient
flowing through both lang_out and lang_emb) against the fp64 reference within the bound of tests/lstm_cases.py (K fixed from the
CPU emulation before any device run), run-to-run bit equality, the launch counter, and the wrappers' host-side rejections.

Observed on the device: see profiles/lang_branch.md."""
import numpy as np
import pytest
import torch

import lstm_cases as lc
import lstm_ref

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(case, H):
    """fp64 and CPU-fp32 nn.LSTM results of a case, computed once and shared (never modified)"""
    key = (case[0], H)
    if key not in _REF:
        c = lc.make_case(case, H)
        _REF[key] = (c, lc.run_torch(c, torch.float64), lc.run_torch(c, torch.float32))
    return _REF[key]


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("case", lc.CASES, ids=[c[0] for c in lc.CASES])
def test_lang_module_fused_against_fp64(dev, case, H):
    from bridgeqa_amd import _ext
    from bridgeqa_amd.lang_module import LangModule
    c, ref, cpu32 = _reference(case, H)
    dirs, layers, lens = (2 if c["bidir"] else 1), c["layers"], c["lens"]
    before = list(_ext.LSTM_CALLS)
    got, dd = lc.run_module(c, dev, LangModule)
    torch.cuda.synchronize()
    assert [a - b for a, b in zip(_ext.LSTM_CALLS, before)] == [layers * dirs, layers * dirs]   # the fused route, fwd and bwd

    out, emb, mask = dd["lang_out"].detach().cpu(), dd["lang_emb"].detach().cpu(), dd["lang_mask"].cpu()
    B, t_out = len(lens), max(lens)
    assert out.shape == (B, t_out, H * dirs) and emb.shape == (B, H * dirs) and mask.shape == (B, t_out)
    for b, n in enumerate(lens):
        assert not out[b, n:].any() and torch.equal(out[b, n:], torch.zeros_like(out[b, n:]))   # exactly zero beyond the length
        assert mask[b].tolist() == [t >= n for t in range(t_out)]
        assert torch.equal(emb[b, :H], out[b, n - 1, :H])            # forward: the state after step len - 1, bit for bit
        if dirs == 2:
            assert torch.equal(emb[b, H:], out[b, 0, H:])            # reverse: the state after step 0

    # the fp64 reference of tests/lstm_ref.py agrees with torch's double nn.LSTM (test_lang_branch_cpu.py); values are held to it
    r_out, r_hn = lstm_ref.lstm_ref(c["x"].numpy(), lens, {k: v.numpy() for k, v in c["params"].items()}, layers, c["bidir"])
    assert np.abs(r_out - ref["out"]).max() < 1e-12
    bad = []
    for k, (err, err_cpu, ulp) in sorted(lc.errors(got, ref, cpu32).items()):
        print("%-24s err %.3e  cpu-fp32 err %.3e  ulp %.3e  ratio %.3f" % (k, err, err_cpu, ulp, lc.ratio(err, err_cpu, ulp)))
        if not err <= lc.K * err_cpu + ulp:
            bad.append((k, err, err_cpu, ulp))
    assert not bad, "beyond K = %.4f CPU-fp32 errors + 1 ulp: %s" % (lc.K, bad)

    got2, dd2 = lc.run_module(c, dev, LangModule)
    for k in got:
        assert np.array_equal(got[k], got2[k]), "two runs differ in %s" % k


@pytest.mark.parametrize("H", [128, 256])
def test_kernel_writes_padding_into_nan_buffers(dev, H, monkeypatch):
    """the outputs start as NaN (torch.empty replaced by a NaN fill): rows beyond the length are zeros the KERNEL wrote"""
    from bridgeqa_amd import _ext
    real_empty = torch.empty

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    lens = torch.tensor(lc.LENS, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(3)
    gx = torch.randn(5, 12, 4 * H, generator=g).to(dev)
    wt = (torch.randn(H, 4 * H, generator=g) / H ** 0.5).to(dev)
    monkeypatch.setattr(_ext.torch, "empty", nan_empty)
    outs = {}
    for rev in (False, True):
        y, h_last, gates, cells = _ext.lstm_fwd(gx, wt, lens, 9, reverse=rev, save=True)
        dgx = _ext.lstm_bwd(torch.ones_like(y), torch.ones_like(h_last), gates, cells, wt.t().contiguous(), lens, reverse=rev)
        outs[rev] = (y, h_last, dgx)
    monkeypatch.undo()
    torch.cuda.synchronize()
    for rev, (y, h_last, dgx) in outs.items():
        assert torch.isfinite(y).all() and torch.isfinite(h_last).all() and torch.isfinite(dgx).all()
        for b, n in enumerate(lc.LENS):
            assert not y[b, n:].any() and not dgx[b, n:].any()
            assert y[b, :n].abs().sum(-1).min() > 0
            assert torch.equal(h_last[b], y[b, 0 if rev else n - 1])


def test_wrappers_reject_before_launching(dev):
    from bridgeqa_amd import _ext
    H = 128
    gx, wt = torch.zeros(2, 4, 4 * H, device=dev), torch.zeros(H, 4 * H, device=dev)
    lens = torch.tensor([4, 2], dtype=torch.int32, device=dev)
    before = list(_ext.LSTM_CALLS)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.lstm_fwd(gx.cpu(), wt, lens, 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        _ext.lstm_fwd(torch.zeros(2, 4 * H, 4, device=dev).transpose(1, 2), wt, lens, 4)
    with pytest.raises(RuntimeError, match="hidden size 100"):
        _ext.lstm_fwd(torch.zeros(2, 4, 400, device=dev), torch.zeros(100, 400, device=dev), lens, 4)
    with pytest.raises(RuntimeError, match="lens"):
        _ext.lstm_fwd(gx, wt, lens[:1], 4)
    with pytest.raises(RuntimeError, match="lens"):
        _ext.lstm_fwd(gx, wt, lens.long(), 4)
    with pytest.raises(RuntimeError, match="t_out"):
        _ext.lstm_fwd(gx, wt, lens, 5)
    gates, cells = torch.zeros(2, 4, 4 * H, device=dev), torch.zeros(2, 4, H, device=dev)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.lstm_bwd(None, None, gates, cells.cpu(), wt.t().contiguous(), lens)
    with pytest.raises(RuntimeError, match="contiguous"):
        _ext.lstm_bwd(None, None, gates, cells, wt.t(), lens)
    with pytest.raises(RuntimeError, match="hidden size 100"):
        _ext.lstm_bwd(None, None, torch.zeros(2, 4, 400, device=dev), torch.zeros(2, 4, 100, device=dev),
                      torch.zeros(400, 100, device=dev), lens)
    assert _ext.LSTM_CALLS == before
