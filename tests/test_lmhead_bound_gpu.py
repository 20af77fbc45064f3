"""The LM head + label-smoothed cross entropy -- the EPI_BIAS_CE epilogue of gemm256_kernel, lmhead_ce_combine_kernel and
lmhead_ce_dlogits_kernel -- held to the per-row / per-element fp64 bounds of tests/lmhead_ref.py: one lost or stale half-tile
record, a target logit read from the bf16 store, a missing eps / V or a vocabulary entry left out fails, where the
whole-tensor norms of tests/test_gemm_gpu.py::test_lm_head_cross_entropy_vs_torch accept it (tests/test_lmhead_bound_cpu.py
shows both).  Every case calls _ext.lmhead_ce_fwd / _ext.lmhead_ce_dlogits directly, moves the results to the CPU and compares
every row and element, the ignored rows and the padding columns included; `not (err <= tol)` fails, so NaN fails.

dlogits runs in two ways: on test-made logits and lse (fp64, rounded once), so that a forward defect cannot hide a backward
one, and chained to the kernel's own forward outputs.  One end-to-end test goes through fusion_ops._LMHeadCE and holds the
three gradient GEMMs behind it as well.  gemm256_kernel accepts D = 64 (one K tile), so the small shapes use it.

The largest |err| / bound per output kind is the last line the module prints (pytest -s).
"""
import time

import pytest
import torch

import lmhead_ref as R

pytestmark = pytest.mark.gpu

KINDS = ("logits", "lse", "loss", "dlogits", "dH", "dW", "db")
_WORST, _COUNT = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print("\nLM-head battery: %.1f s; elements held per output kind: %s" % (
        time.time() - t0, "  ".join("%s %d" % (k, _COUNT.get(k, 0)) for k in KINDS)))
    print("largest |err| / bound per output kind: " + "  ".join("%s %.3g" % (k, _WORST.get(k, 0.0)) for k in KINDS))


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
        _COUNT[kind] = _COUNT.get(kind, 0) + ref.numel()
        print("%s %s: |err| / bound %.3g over %d" % (self.name, what or kind, ratio, ref.numel()))
        if msg:
            self.fails.append("%s %s: %s" % (self.name, what or kind, msg))

    def true(self, cond, msg):
        if not cond:
            self.fails.append("%s: %s" % (self.name, msg))

    def assert_ok(self):
        assert not self.fails, "\n".join(self.fails)


def _case_id(c):
    return "R%d-D%d-V%d%s" % (c[0], c[1], c[2], "-shift%+g" % c[3] if c[3] else "")


def _to(dev, *ts):
    return [t.to(dev) for t in ts]


def _forward(ext, dev, d, V, eps):
    h, w, bp, tg = _to(dev, d["h"], d["w"], d["bias_pad"], d["tgt"])
    return ext.lmhead_ce_fwd(h, w, bp, tg, V, eps)


def _hold_forward(hold, f, tgt, V, eps, logits, loss, lse):
    """stored logits (every column: the padding is 0 exactly), lse of every row, loss of every row (ignored: 0 exactly)"""
    Rr = tgt.numel()
    x = logits.cpu()
    hold.true(x.shape == (Rr, R.padded(V)) and x.dtype == torch.bfloat16 and loss.shape == (Rr,) and lse.shape == (Rr,), "shapes")
    hold("logits", x[:, :V], f["z"], f["tol_x"])
    hold.true(not bool(x[:, V:].float().any()), "padding columns of the logits are not exactly 0")
    hold("lse", lse, f["L"], f["tol_L"])
    ref, tol, valid = R.loss(f, tgt, eps)
    hold("loss", loss, ref, tol)
    hold.true(bool((loss.cpu()[~valid] == 0).all()), "an ignored row's loss is not exactly 0")


def _hold_dlogits(hold, dl, x, l, g, tgt, V, eps):
    ref, tol, _ = R.dlogits(x, l, g, tgt, V, eps)
    out = dl.cpu()
    hold.true(out.shape == x.shape and out.dtype == torch.bfloat16, "dlogits shape / type")
    hold("dlogits", out, ref, tol)
    hold.true(not bool(out[tgt < 0].float().any()) and not bool(out[:, V:].float().any()),
              "dlogits of an ignored row or a padding column are not exactly 0")


# ---- forward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", R.SMOOTHINGS)
@pytest.mark.parametrize("case", R.CASES, ids=_case_id)
def test_forward(dev, ext, case, eps):
    V = case[2]
    d, f = R.inputs(*case), R.forward_of(*case)
    hold = _Hold("fwd-%s-eps%g" % (_case_id(case), eps))
    _hold_forward(hold, f, d["tgt"], V, eps, *_forward(ext, dev, d, V, eps))
    hold.assert_ok()


# ---- dlogits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", R.SMOOTHINGS)
@pytest.mark.parametrize("case", R.CASES, ids=_case_id)
def test_dlogits_on_test_made_logits_and_lse(dev, ext, case, eps):
    """x = the fp64 logits rounded once to bf16 (the padding columns hold 1: the kernel must store zeros there whatever it
    finds), l = the fp64 lse rounded once to fp32"""
    V = case[2]
    d, f = R.inputs(*case), R.forward_of(*case)
    x, l = R.made_forward_outputs(f, V)
    xd, ld, tg, g = _to(dev, x, l, d["tgt"], d["g"])
    dl = ext.lmhead_ce_dlogits(xd, ld, tg, g, V, eps)
    hold = _Hold("dlogits-%s-eps%g" % (_case_id(case), eps))
    hold.true(dl.data_ptr() == xd.data_ptr(), "dlogits is not formed in place")
    _hold_dlogits(hold, dl, x, l, d["g"], d["tgt"], V, eps)
    hold.assert_ok()


@pytest.mark.parametrize("case,eps", [(c, R.SMOOTHINGS[k % 3]) for k, c in enumerate(R.CASES)], ids=lambda v: _case_id(v) if isinstance(v, tuple) else "eps%g" % v)
def test_dlogits_chained_to_the_kernels_own_forward(dev, ext, case, eps):
    """the kernel's own stored logits and lse go into its dlogits and into the reference"""
    V = case[2]
    d = R.inputs(*case)
    logits, loss, lse = _forward(ext, dev, d, V, eps)
    x, l = logits.cpu().clone(), lse.cpu().clone()
    dl = ext.lmhead_ce_dlogits(logits, lse, d["tgt"].to(dev), d["g"].to(dev), V, eps)
    hold = _Hold("chained-%s-eps%g" % (_case_id(case), eps))
    _hold_dlogits(hold, dl, x, l, d["g"], d["tgt"], V, eps)
    hold.assert_ok()


# ---- the production shape -------------------------------------------------------------------------------------------------------
def test_production_shape_forward_and_chained_dlogits(dev, ext):
    """(160 rows, D 768, V 30524): 240 records per row -- four serial trips of the combine, the last one ragged -- and 4 padding
    columns; once, with the smoothing the model trains with"""
    case, eps = R.PRODUCTION + (0.0,), 0.1
    V = case[2]
    d, f = R.inputs(*case), R.forward_of(*case)
    logits, loss, lse = _forward(ext, dev, d, V, eps)
    hold = _Hold("production")
    _hold_forward(hold, f, d["tgt"], V, eps, logits, loss, lse)
    x, l = logits.cpu().clone(), lse.cpu().clone()
    dl = ext.lmhead_ce_dlogits(logits, lse, d["tgt"].to(dev), d["g"].to(dev), V, eps)
    _hold_dlogits(hold, dl, x, l, d["g"], d["tgt"], V, eps)
    hold.assert_ok()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,L,D,V", [(3, 6, 256, 200), (1, 257, 64, 130)])
def test_end_to_end_through_the_autograd_function(dev, B, L, D, V, with_bias):
    """fusion_ops._LMHeadCE.apply, then a backward with per-row weights that are non-zero on the ignored positions too.  The
    function shifts the labels (position t predicts label t + 1; a sequence's last position is ignored).  The forward's logits
    buffer and lse are read from the saved tensors; after the backward that buffer holds dlogits (consumed in place): the
    kernel's own dl, held to the dlogits bound at a copy of the logits taken before, and the operand the three gradients are
    held at -- dH (fp32 over the Vp-long cut contraction, then bf16), dW[:V] (fp32, contraction R), db (fp32 column sums)."""
    from bridgeqa_amd import fusion_ops as ops
    Rr, eps = B * L, 0.1
    d = R.inputs(Rr, D, V)
    tgt = d["tgt"].view(B, L).clone()
    labels = torch.full((B, L), R.IGNORE, dtype=torch.int64)
    labels[:, 1:] = tgt[:, :-1]
    tgt[:, -1] = R.IGNORE
    tgt = tgt.view(-1)
    bias = d["bias"] if with_bias else None
    f = R.forward(d["h"], d["w"], bias)
    hold = _Hold("e2e-%d-%d-%d-%s" % (Rr, D, V, "bias" if with_bias else "nobias"))
    prev = ops.set_compute_dtype(torch.bfloat16)
    try:
        h = d["h"].view(B, L, D).to(dev).requires_grad_(True)
        w = torch.nn.Parameter(d["w"].float().to(dev))
        b = torch.nn.Parameter(bias.to(dev)) if with_bias else None
        logits, loss = ops._LMHeadCE.apply(h, w, b, labels.to(dev), eps)
        hold.true(logits.shape == (B, L, V) and loss.shape == (B, L), "shapes")
        _, _, buf, lse, tg = loss.grad_fn.saved_tensors
        hold.true(buf.shape == (Rr, R.padded(V)) and logits.data_ptr() == buf.data_ptr() and torch.equal(tg.cpu().view(-1), tgt.to(torch.int32)),
                  "the saved logits buffer / targets are not the ones expected")
        x, l = buf.cpu().clone(), lse.cpu().clone()
        _hold_forward(hold, f, tgt, V, eps, buf, loss.detach().view(-1), lse)
        (loss * d["g"].view(B, L).to(dev)).sum().backward()
        dl = buf.cpu()
    finally:
        ops.set_compute_dtype(prev)
    _hold_dlogits(hold, dl, x, l, d["g"], tgt, V, eps)
    (dh, tol_dh), (dw, tol_dw), (db, tol_db) = R.grads(dl, d["h"], d["w"], V)
    hold.true(h.grad.dtype == torch.bfloat16 and w.grad.dtype == torch.float32 and w.grad.shape == (V, D), "gradient types")
    hold("dH", h.grad.view(Rr, D), dh, tol_dh)
    hold("dW", w.grad, dw, tol_dw)
    if with_bias:
        hold("db", b.grad, db, tol_db)
    hold.assert_ok()
