"""The kernels of csrc/mcan.hip on the device: each held per element to the fp64 bound of tests/mcan_ref.py (a NaN anywhere fails),
bit-identical between two runs, exact where the arithmetic is exact (a constant row gives b2, hidden dlogits are 0); the modules
of bridgeqa_amd/mcan_module.py with the switch on against off under one seed, both measured against the same computation in
fp64; the route proven by counting device kernels under torch.profiler; LayerNorm forward + backward captured in one graph.

Measured on an MI355X (largest |err| / bound per output, module-level errors): profiles/mcan_rows.md."""
import copy

import pytest
import torch
import torch.nn as nn

import mcan_ref as R

_old_attflat_tail = R.composition_attflat_tail

pytestmark = pytest.mark.gpu


def _held(name, out, ref, tol, rows=None):
    if rows is not None:
        out, ref, tol = out.cpu()[rows], ref[rows], tol[rows]
    r, msg = R.excess(out, ref, tol)
    print("%-10s |err| / bound %.3g" % (name, r))
    assert msg is None, "%s: %s" % (name, msg)


def _to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


@pytest.fixture()
def fused():
    from bridgeqa_amd import mcan_module
    prev = mcan_module.set_fused(True)
    yield mcan_module
    mcan_module.set_fused(prev)


# ---- the four kernels, per element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, H", R.LN_SHAPES)
@pytest.mark.parametrize("with_s", [True, False])
def test_layernorm_forward_is_within_the_bound_and_reproducible(dev, M, H, with_s):
    from bridgeqa_amd import _ext
    d = R.ln_inputs(M, H)
    s_host = d["s"] if with_s else None
    x, s, a2, b2 = _to(dev, d["x"], s_host, d["a2"], d["b2"])
    y, mean, sigma = _ext.mcan_ln_fwd(x, s, a2, b2, R.EPS)
    y2, mean2, sigma2 = _ext.mcan_ln_fwd(x, s, a2, b2, R.EPS)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(sigma, sigma2)
    ref = R.ln_forward(d["x"], s_host, d["a2"], d["b2"])
    rows = R.regular_rows(M)
    _held("y", y, ref["y"], ref["tol_y"], rows)
    _held("mean", mean, ref["mean"], ref["tol_mean"], rows)
    _held("sigma", sigma, ref["sigma"], ref["tol_sigma"], rows)
    assert torch.isfinite(y).all()
    if M > R.CONST_ROW:
        assert torch.equal(y[R.CONST_ROW].cpu(), d["b2"]) and float(sigma[R.CONST_ROW]) == 0.0


@pytest.mark.parametrize("M, H", R.LN_SHAPES)
@pytest.mark.parametrize("with_s", [True, False])
def test_layernorm_backward_is_within_the_bound_and_reproducible(dev, M, H, with_s):
    """M = 67 (66 rows without the constant one) is 17 workgroups: the slab fold adds more than one partial"""
    from bridgeqa_amd import _ext
    b = R.ln_bwd_inputs(M, H, with_s)
    dy, x, s, a2, mean, sigma = _to(dev, b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"])
    dz, dab = _ext.mcan_ln_bwd(dy, x, s, a2, mean, sigma, R.EPS)
    dz2, dab2 = _ext.mcan_ln_bwd(dy, x, s, a2, mean, sigma, R.EPS)
    assert torch.equal(dz, dz2) and torch.equal(dab, dab2)
    ref = R.ln_backward(b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"])
    _held("dz", dz, ref["dz"], ref["tol_dz"])
    _held("da2", dab[0], ref["da2"], ref["tol_da2"])
    _held("db2", dab[1], ref["db2"], ref["tol_db2"])


def test_layernorm_constant_row_has_a_nan_gradient(dev):
    """sigma = 0 is not guarded in the backward either: inf 0, as autograd of the composition gives"""
    from bridgeqa_amd import _ext
    d = R.ln_inputs(5, 64)
    x, s, a2, b2, dy = _to(dev, d["x"], d["s"], d["a2"], d["b2"], d["dy"])
    _, mean, sigma = _ext.mcan_ln_fwd(x, s, a2, b2, R.EPS)
    dz, dab = _ext.mcan_ln_bwd(dy, x, s, a2, mean, sigma, R.EPS)
    rows = R.regular_rows(5).to(dev)
    assert torch.isnan(dz[R.CONST_ROW]).all() and torch.isfinite(dz[rows]).all() and torch.isfinite(dab).all()


@pytest.mark.parametrize("B, N, G, H", R.POOL_SHAPES)
@pytest.mark.parametrize("kind", R.MASKS)
def test_pool_is_within_the_bound_and_reproducible(dev, B, N, G, H, kind):
    from bridgeqa_amd import _ext
    d = R.pool_inputs(B, N, G, H)
    hide = R.pool_hide(B, N, kind)
    x, logits, dout = _to(dev, d["x"], d["logits"], d["dout"])
    hide_d = hide.to(torch.uint8).to(dev) if hide is not None else None
    out, p = _ext.attflat_pool_fwd(x, logits, hide_d)
    out2, p2 = _ext.attflat_pool_fwd(x, logits, hide_d)
    assert torch.equal(out, out2) and torch.equal(p, p2)
    ref = R.pool_forward(d["x"], d["logits"], hide)
    _held("p", p, ref["p"], ref["tol_p"])
    _held("out", out, ref["out"], ref["tol_out"])
    if hide is not None:
        assert (p[1] == p[1, 0, 0]).all()                       # a fully hidden sample pools uniformly
    p32 = R.pool_p32(d["logits"], hide)
    p_d = p32.to(dev)
    dx, dl = _ext.attflat_pool_bwd(dout, x, p_d, hide_d)
    dx2, dl2 = _ext.attflat_pool_bwd(dout, x, p_d, hide_d)
    assert torch.equal(dx, dx2) and torch.equal(dl, dl2)
    ref = R.pool_backward(d["dout"], d["x"], p32, hide)
    _held("dx", dx, ref["dx"], ref["tol_dx"])
    _held("dl", dl, ref["dl"], ref["tol_dl"])
    if hide is not None:
        assert (dl.cpu()[hide] == 0).all()


def test_ineligible_sizes_raise(dev):
    from bridgeqa_amd import _ext
    v = torch.zeros(96, device=dev)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.mcan_ln_fwd(torch.zeros(4, 96, device=dev), None, v, v, R.EPS)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.attflat_pool_fwd(torch.zeros(2, 1025, 64, device=dev), torch.zeros(2, 1025, 1, device=dev), None)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.attflat_pool_fwd(torch.zeros(2, 8, 64, device=dev), torch.zeros(2, 8, 5, device=dev), None)


# ---- the modules: switch on against off, both against fp64 ----------------------------------------------------------------------
class _Masks(object):
    """records every nn.Dropout's keep mask and scale in call order (record), or applies the recorded ones to a module whose
    dropouts are switched off (replay): the fp64 run then sees the masks the fp32 runs drew"""

    def __init__(self, module):
        self.drops = [m for m in module.modules() if isinstance(m, nn.Dropout)]
        self.masks, self.at, self.handles = [], 0, []

    def record(self):
        def hook(m, inp, out):
            keep = out != 0
            cands = [torch.tensor(1.0 / (1.0 - m.p), dtype=torch.float32), torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(m.p))]
            scale = [float(c) for c in cands if torch.equal(out, inp[0] * keep * c.to(out.device))]
            assert scale, "nn.Dropout scaled by neither rounding of 1 / (1 - p)"
            self.masks.append((keep, scale[0]))
        self.handles = [m.register_forward_hook(hook) for m in self.drops]
        return self

    def replay(self, masks):
        def hook(m, inp, out):
            keep, scale = masks[self.at]
            self.at += 1
            return inp[0] * keep * scale
        for m in self.drops:
            m.eval()
        self.handles = [m.register_forward_hook(hook) for m in self.drops]
        return self

    def remove(self):
        for h in self.handles:
            h.remove()


def _run(module, inputs, run, gout):
    """forward + backward; returns {name: tensor} of the output, the input gradients and every parameter gradient"""
    ins = [t.detach().clone().requires_grad_(True) if t.is_floating_point() else t for t in inputs]
    for p in module.parameters():
        p.grad = None
    out = run(module, *ins)
    out.backward(gout.to(out.dtype))
    res = {"out": out.detach()}
    res.update({"d_in%d" % i: t.grad for i, t in enumerate(ins) if t.is_floating_point()})
    res.update({"d_" + n: p.grad for n, p in module.named_parameters()})
    return res


def _three_routes(mcan_module, module, inputs, run, gout, seed):
    """(off, on, truth): the fp32 composition, the fp32 fused route, fp64 with the masks the composition drew"""
    prev = mcan_module.set_fused(False)
    try:
        rec = _Masks(module).record()
        torch.manual_seed(seed)
        off = _run(module, inputs, run, gout)
        rec.remove()
        mcan_module.set_fused(True)
        rec_on = _Masks(module).record()
        torch.manual_seed(seed)
        on = _run(module, inputs, run, gout)
        rec_on.remove()
        assert len(rec.masks) == len(rec_on.masks) and all(torch.equal(a[0], b[0]) for a, b in zip(rec.masks, rec_on.masks)), \
            "the two routes drew different dropout masks under one seed"
        mcan_module.set_fused(False)
        exact = copy.deepcopy(module).double()
        rep = _Masks(exact).replay(rec.masks)
        truth = _run(exact, [t.double() if t.is_floating_point() else t for t in inputs], run, gout)
        rep.remove()
        assert rep.at == len(rec.masks)
    finally:
        mcan_module.set_fused(prev)
    return off, on, truth


def _allowance(what, off, on, truth):
    """the fused route may err at most twice what the composition errs, per tensor, in max-norm against fp64"""
    assert set(off) == set(on) == set(truth)
    bad = []
    for k in sorted(truth):
        e_off = float((off[k].double() - truth[k]).abs().max())
        e_on = float((on[k].double() - truth[k]).abs().max())
        print("%s %-34s |truth| %.3e  err off %.3e  err on %.3e" % (what, k, float(truth[k].abs().max()), e_off, e_on))
        if not e_on <= 2.0 * e_off:
            bad.append((k, e_off, e_on))
    assert not bad, "%s: the fused route errs more than twice the composition's own error: %s" % (what, bad)


def test_sga_layer_fused_against_composition_under_one_seed(dev):
    """Measured on an MI355X, max-norm error against fp64, composition / fused: output 1.47e-6 / 1.51e-6, gradient of x 1.60e-6 /
    1.35e-6, norm3.b_2 1.79e-6 / 1.78e-6, the largest error ffn.mlp.linear.weight 1.36e-5 / 1.36e-5, the largest ratio 1.54
    (mhatt1.linear_merge.bias 4.65e-6 / 7.14e-6); all 29 tensors in profiles/mcan_rows.md."""
    from bridgeqa_amd import _ext, mcan_module
    torch.manual_seed(5)
    B, K, T, H = 2, 37, 9, 256
    sga = mcan_module.SGA(H, num_heads=8, pdrop=0.1).to(dev).train()
    with torch.no_grad():
        for n in (sga.norm1, sga.norm2, sga.norm3):
            n.a_2.uniform_(0.5, 1.5)
            n.b_2.normal_(0, 0.1)
    x, y = torch.randn(B, K, H, device=dev), torch.randn(B, T, H, device=dev)
    y_mask = torch.zeros(B, 1, 1, T, dtype=torch.bool, device=dev)
    y_mask[1, :, :, T - 2:] = True
    gout = torch.randn(B, K, H, device=dev)
    calls = list(_ext.MCAN_CALLS)
    off, on, truth = _three_routes(mcan_module, sga, [x, y, y_mask], lambda m, a, b, mk: m(a, b, None, mk), gout, 17)
    assert [p - q for p, q in zip(_ext.MCAN_CALLS, calls)] == [3, 3, 0, 0]          # the fused run, and only it, took the kernels
    _allowance("SGA", off, on, truth)


def test_attflat_fused_against_composition_under_one_seed(dev):
    """Measured on an MI355X, composition / fused: output 1.05e-7 / 1.23e-7, gradient of x 1.04e-7 / 1.04e-7, the largest ratio
    1.65 (linear_merge.weight 3.78e-7 / 6.23e-7)."""
    from bridgeqa_amd import _ext, mcan_module
    torch.manual_seed(6)
    B, K, H = 2, 37, 256
    flat = mcan_module.AttFlat(H, flat_mlp_size=512, flat_glimpses=1, flat_out_size=1024, pdrop=0.1).to(dev).train()
    x = torch.randn(B, K, H, device=dev)
    mask = torch.zeros(B, 1, 1, K, dtype=torch.bool, device=dev)
    mask[0, :, :, K - 12:] = True
    gout = torch.randn(B, 1024, device=dev)
    calls = list(_ext.MCAN_CALLS)
    off, on, truth = _three_routes(mcan_module, flat, [x, mask], lambda m, a, mk: m(a, mk), gout, 18)
    assert [p - q for p, q in zip(_ext.MCAN_CALLS, calls)] == [0, 0, 1, 1]
    _allowance("AttFlat", off, on, truth)


# ---- proof of the route: device kernels under the profiler ----------------------------------------------------------------------
def _kernels(fn):
    """(fn's result, the device kernels of one call)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return res, [n for n in names if "emcpy" not in n and "emset" not in n]


def test_layernorm_route_by_kernel_count(dev, fused):
    M, H = 67, 256
    d = R.ln_bwd_inputs(M, H)
    x, s, dy = [t.requires_grad_(True) for t in _to(dev, d["x"], d["s"])] + [d["dy"].to(dev)]
    m = fused.LayerNorm(H).to(dev)
    leaves = (x, s, m.a_2, m.b_2)
    for route in (True, False):                                   # one warm-up of either route outside the profiler
        fused.set_fused(route)
        torch.autograd.grad(m(x, s), leaves, dy)
    fused.set_fused(True)
    y_on, k_fwd_on = _kernels(lambda: m(x, s))
    _, k_bwd_on = _kernels(lambda: torch.autograd.grad(y_on, leaves, dy))
    fused.set_fused(False)
    y_off, k_fwd_off = _kernels(lambda: m(x, s))
    _, k_bwd_off = _kernels(lambda: torch.autograd.grad(y_off, leaves, dy))
    print("LayerNorm kernels: forward %d (composition %d), backward %d (composition %d)" % (
        len(k_fwd_on), len(k_fwd_off), len(k_bwd_on), len(k_bwd_off)))
    assert k_fwd_off and k_bwd_off, "the profiler reported no device kernels at all -- the route cannot be proven"
    assert len(k_fwd_on) == 1 and "mcan_ln_fwd_kernel" in k_fwd_on[0], k_fwd_on
    assert 1 <= len(k_bwd_on) <= 2 and any("mcan_ln_bwd_kernel" in k for k in k_bwd_on), k_bwd_on
    assert len(k_fwd_on) < len(k_fwd_off) and len(k_bwd_on) < len(k_bwd_off)


def test_pool_route_by_kernel_count(dev, fused):
    B, N, G, H = 3, 37, 2, 256
    d = R.pool_inputs(B, N, G, H)
    hide = R.pool_hide(B, N, "mixed").to(dev)
    x, logits = [t.requires_grad_(True) for t in _to(dev, d["x"], d["logits"])]
    dout = d["dout"].to(dev)
    hide8, mask = hide.view(torch.uint8), hide.view(B, 1, 1, N)
    on = lambda: fused._AttFlatPoolFn.apply(x, logits, hide8)
    off = lambda: _old_attflat_tail(logits, x, mask, G)
    for f in (on, off):
        torch.autograd.grad(f(), (x, logits), dout)
    o_on, k_fwd_on = _kernels(on)
    _, k_bwd_on = _kernels(lambda: torch.autograd.grad(o_on, (x, logits), dout))
    o_off, k_fwd_off = _kernels(off)
    _, k_bwd_off = _kernels(lambda: torch.autograd.grad(o_off, (x, logits), dout))
    print("AttFlat pool kernels: forward %d (composition %d), backward %d (composition %d)" % (
        len(k_fwd_on), len(k_fwd_off), len(k_bwd_on), len(k_bwd_off)))
    assert k_fwd_off and k_bwd_off, "the profiler reported no device kernels at all -- the route cannot be proven"
    assert len(k_fwd_on) == 1 and "mcan_pool_fwd_kernel" in k_fwd_on[0], k_fwd_on
    assert len(k_bwd_on) == 1 and "mcan_pool_bwd_kernel" in k_bwd_on[0], k_bwd_on
    assert len(k_fwd_on) < len(k_fwd_off) and len(k_bwd_on) < len(k_bwd_off)


# ---- capture ----------------------------------------------------------------------------------------------------------------
def test_layernorm_forward_and_backward_replay_from_one_graph(dev, fused):
    """forward + backward captured on one stream (no fork) and replayed twice is bitwise the eager result.  The eager pass runs
    on the stream of the capture: autograd's AccumulateGrad nodes remember the stream they were born on, and a captured backward
    that hands a gradient to a node born on another stream draws that stream into the capture, which then cannot end."""
    M, H = 67, 256
    d = R.ln_bwd_inputs(M, H)
    x, s, dy = [t.requires_grad_(True) for t in _to(dev, d["x"], d["s"])] + [d["dy"].to(dev)]
    m = fused.LayerNorm(H).to(dev)
    with torch.no_grad():
        m.a_2.copy_(d["a2"])
    leaves = (x, s, m.a_2, m.b_2)

    def fwd_bwd():
        y = m(x, s)
        return [y.detach()] + list(torch.autograd.grad(y, leaves, dy))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eager = [t.clone() for t in fwd_bwd()]
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = fwd_bwd()
    torch.cuda.synchronize(dev)
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip(outs, eager):
            assert torch.equal(got, want)
