"""The kernels of csrc/mhatt.hip on the device: every output held per element to the fp64 bound of tests/mhatt_ref.py (a NaN anywhere
fails), bit-identical between two runs, exact where the tolerance is 0; the modules of bridgeqa_amd/mcan_module.py with the
attention switch on against off under one seed, both measured against the same computation in fp64, once over the torch
LayerNorm and once over the row kernels of csrc/mcan.hip; the route proven by counting device kernels under torch.profiler;
MHAtt forward + backward in eval mode captured in one graph.

Measured on an MI355X (largest |err| / bound per output, module-level errors, kernel counts): profiles/mhatt.md."""
import copy

import pytest
import torch
import torch.nn as nn

import mhatt_ref as R

pytestmark = pytest.mark.gpu


def _held(name, out, ref, tol):
    r, msg = R.excess(out, ref, tol)
    print("mhatt-ratio %-4s %.3g" % (name, r))
    assert msg is None, "%s: %s" % (name, msg)


def _to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


@pytest.fixture()
def att_on():
    from bridgeqa_amd import mcan_module
    prev = mcan_module.set_fused_attention(True)
    yield mcan_module
    mcan_module.set_fused_attention(prev)


# ---- the kernels, per element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_and_backward_are_within_the_bound_and_reproducible(dev, case):
    from bridgeqa_amd import _ext
    d, fwd, p32, bwd = R.reference(case)
    (B, heads, Nq, Nk, hd), kind, kp = case
    q, k, v, dout, keep = _to(dev, d["q"], d["k"], d["v"], d["dout"], d["keep"])
    hide = d["hide"].to(torch.uint8).to(dev) if d["hide"] is not None else None
    out, p = _ext.mhatt_fwd(q, k, v, hide, keep, heads)
    out2, p2 = _ext.mhatt_fwd(q, k, v, hide, keep, heads)
    assert torch.equal(out, out2) and torch.equal(p, p2)
    _held("p", p, fwd["p"], fwd["tol_p"])
    _held("out", out, fwd["out"], fwd["tol_out"])
    p_d = p32.to(dev)                                           # the backward is fed the host's p, the one its reference reads
    dq, dk, dv = _ext.mhatt_bwd(dout, q, k, v, p_d, hide, keep, heads)
    dq2, dk2, dv2 = _ext.mhatt_bwd(dout, q, k, v, p_d, hide, keep, heads)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    _held("dq", dq, bwd["dq"], bwd["tol_dq"])
    _held("dk", dk, bwd["dk"], bwd["tol_dk"])
    _held("dv", dv, bwd["dv"], bwd["tol_dv"])
    if kind == "mixed":
        assert (p[1] == p[1, :, :, :1]).all()                    # a fully hidden sample: one value of p per row
        assert (dq[1] == 0).all() and (dk[1] == 0).all()
    if Nk == 1:
        assert (p == 1).all() and (dq == 0).all() and (dk == 0).all()


def test_ineligible_sizes_raise(dev):
    from bridgeqa_amd import _ext
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.mhatt_fwd(z(2, 4, 96), z(2, 5, 96), z(2, 5, 96), None, None, 2)                     # d = 48
    with pytest.raises(RuntimeError, match="not built"):
        _ext.mhatt_fwd(z(2, 4, 32), z(2, 1025, 32), z(2, 1025, 32), None, None, 1)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.mhatt_fwd(z(2, 1025, 32), z(2, 4, 32), z(2, 4, 32), None, None, 1)
    with pytest.raises(RuntimeError, match="not built"):
        _ext.mhatt_bwd(z(2, 4, 96), z(2, 4, 96), z(2, 5, 96), z(2, 5, 96), z(2, 2, 4, 5), None, None, 2)
    with pytest.raises(RuntimeError, match="shape"):
        _ext.mhatt_fwd(z(2, 4, 64), z(2, 5, 64), z(2, 5, 64), None, z(2, 2, 4, 4), 2)             # keep of the wrong shape


# ---- the modules: attention switch on against off, both against fp64 ------------------------------------------------------------
class _Masks(object):
    """records every nn.Dropout's keep mask, the positions where its input was non-zero, and its scale, in call order (record),
    or applies the recorded ones to a module whose dropouts are switched off (replay): the fp64 run then sees the masks the fp32
    runs drew"""

    def __init__(self, module):
        self.named = [(n, m) for n, m in module.named_modules() if isinstance(m, nn.Dropout)]
        self.masks, self.at, self.handles = [], 0, []

    def record(self):
        def hook(name):
            def f(m, inp, out):
                keep = out != 0
                cands = [torch.tensor(1.0 / (1.0 - m.p), dtype=torch.float32), torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(m.p))]
                scale = [float(c) for c in cands if torch.equal(out, inp[0] * keep * c.to(out.device))]
                assert scale, "nn.Dropout scaled by neither rounding of 1 / (1 - p)"
                self.masks.append((keep, scale[0], inp[0] != 0, name))
            return f
        self.handles = [m.register_forward_hook(hook(n)) for n, m in self.named]
        return self

    def replay(self, masks):
        def hook(m, inp, out):
            keep, scale = masks[self.at][:2]
            self.at += 1
            return inp[0] * keep * scale
        for _, m in self.named:
            m.eval()
        self.handles = [m.register_forward_hook(hook) for _, m in self.named]
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


def _three_routes(mcan_module, module, inputs, run, gout, seed, sites):
    """(off, on, truth): the fp32 composition of the attention core, the fp32 kernels, fp64 with the masks the composition drew.
    MHATT_CALLS moves by `sites` each way in the `on` run and not at all in the others."""
    from bridgeqa_amd import _ext
    prev = mcan_module.set_fused_attention(False)
    try:
        calls = list(_ext.MHATT_CALLS)
        rec = _Masks(module).record()
        torch.manual_seed(seed)
        off = _run(module, inputs, run, gout)
        rec.remove()
        assert _ext.MHATT_CALLS == calls
        mcan_module.set_fused_attention(True)
        rec_on = _Masks(module).record()
        torch.manual_seed(seed)
        on = _run(module, inputs, run, gout)
        rec_on.remove()
        assert [a - b for a, b in zip(_ext.MHATT_CALLS, calls)] == [sites, sites]
        calls = list(_ext.MHATT_CALLS)
        assert [m[3] for m in rec.masks] == [m[3] for m in rec_on.masks]
        for (keep, scale, seen, name), (keep_on, scale_on, _, _) in zip(rec.masks, rec_on.masks):
            # a hidden key's p is 0 in the composition and hides its mask bit: compare where the composition's input was non-zero
            assert scale == scale_on and torch.equal(keep[seen], keep_on[seen]), \
                "%s drew different dropout masks on the two routes under one seed" % name
        mcan_module.set_fused_attention(False)
        exact = copy.deepcopy(module).double()
        rep = _Masks(exact).replay(rec.masks)
        truth = _run(exact, [t.double() if t.is_floating_point() else t for t in inputs], run, gout)
        rep.remove()
        assert rep.at == len(rec.masks) and _ext.MHATT_CALLS == calls
    finally:
        mcan_module.set_fused_attention(prev)
    return off, on, truth


def _allowance(what, off, on, truth):
    """per tensor, in max-norm against fp64: err_on <= 2 err_off + u max|truth| -- the 2 is the project's own allowance
    (tests/test_mcan_rows_gpu.py), the floor one rounding of the tensor's largest entry.  The gradients of the key projections'
    biases are printed and left out: they are exactly zero in real arithmetic (softmax is invariant to a per-row shift), rounding
    noise on either route; their terms, dk, are held per element by the kernel tests."""
    assert set(off) == set(on) == set(truth)
    bad = []
    for k in sorted(truth):
        top = float(truth[k].abs().max())
        e_off = float((off[k].double() - truth[k]).abs().max())
        e_on = float((on[k].double() - truth[k]).abs().max())
        skipped = k.endswith("linear_k.bias")
        print("mhatt-module %s %-34s |truth| %.3e  err off %.3e  err on %.3e%s" % (what, k, top, e_off, e_on, "  (not held)" if skipped else ""))
        if not skipped and not e_on <= 2.0 * e_off + R.U * top:
            bad.append((k, e_off, e_on))
    assert not bad, "%s: the attention kernels err more than twice the composition's own error: %s" % (what, bad)


@pytest.mark.parametrize("rows_fused", [False, True], ids=["torch_rows", "row_kernels"])
def test_sga_and_sa_fused_attention_against_composition_under_one_seed(dev, rows_fused):
    from bridgeqa_amd import _ext, mcan_module
    prev = mcan_module.set_fused(rows_fused)
    try:
        torch.manual_seed(5)
        B, K, T, H = 2, 37, 9, 256
        sga = mcan_module.SGA(H, num_heads=8, pdrop=0.1).to(dev).train()
        sa = mcan_module.SA(H, num_heads=8, pdrop=0.1).to(dev).train()
        with torch.no_grad():
            for n in (sga.norm1, sga.norm2, sga.norm3, sa.norm1, sa.norm2):
                n.a_2.uniform_(0.5, 1.5)
                n.b_2.normal_(0, 0.1)
        x, y = torch.randn(B, K, H, device=dev), torch.randn(B, T, H, device=dev)
        y_mask = torch.zeros(B, 1, 1, T, dtype=torch.bool, device=dev)
        y_mask[1, :, :, T - 2:] = True
        x_mask = torch.zeros(B, 1, 1, K, dtype=torch.bool, device=dev)
        x_mask[0, :, :, K - 12:] = True
        gout = torch.randn(B, K, H, device=dev)
        calls = list(_ext.MHATT_CALLS)
        off, on, truth = _three_routes(mcan_module, sga, [x, y, y_mask], lambda m, a, b, mk: m(a, b, None, mk), gout, 17, 2)
        _allowance("SGA/%s" % ("row_kernels" if rows_fused else "torch_rows"), off, on, truth)
        off, on, truth = _three_routes(mcan_module, sa, [x, x_mask], lambda m, a, mk: m(a, mk), gout, 18, 1)
        _allowance("SA/%s" % ("row_kernels" if rows_fused else "torch_rows"), off, on, truth)
        assert [p - q for p, q in zip(_ext.MHATT_CALLS, calls)] == [3, 3]
    finally:
        mcan_module.set_fused(prev)


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


def _core_composition(q, k, v, mask, heads):
    """MHAtt.forward between the three linears and linear_merge, as the composition runs it (no dropout: eval, or p = 0)"""
    import math
    qh, kh, vh = R.split(q, heads), R.split(k, heads), R.split(v, heads)
    scores = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(qh.size(-1))
    if mask is not None:
        scores = scores.masked_fill(mask, -1e9)
    ctx = torch.matmul(torch.softmax(scores, dim=-1), vh)
    return ctx.transpose(1, 2).contiguous().view(q.shape)


def test_route_by_kernel_count(dev, att_on):
    d = R.inputs((3, 8, 37, 9, 32), "mixed", False)
    heads = d["heads"]
    q, k, v = [t.requires_grad_(True) for t in _to(dev, d["q"], d["k"], d["v"])]
    dout = d["dout"].to(dev)
    hide = d["hide"].to(dev)
    hide8, mask = hide.view(torch.uint8), hide.view(3, 1, 1, 9)
    on = lambda: att_on._MHAttCoreFn.apply(q, k, v, hide8, None, heads)
    off = lambda: _core_composition(q, k, v, mask, heads)
    for f in (on, off):
        torch.autograd.grad(f(), (q, k, v), dout)
    o_on, k_fwd_on = _kernels(on)
    _, k_bwd_on = _kernels(lambda: torch.autograd.grad(o_on, (q, k, v), dout))
    o_off, k_fwd_off = _kernels(off)
    _, k_bwd_off = _kernels(lambda: torch.autograd.grad(o_off, (q, k, v), dout))
    print("mhatt-kernels forward %d (composition %d), backward %d (composition %d)" % (
        len(k_fwd_on), len(k_fwd_off), len(k_bwd_on), len(k_bwd_off)))
    assert k_fwd_off and k_bwd_off, "the profiler reported no device kernels at all -- the route cannot be proven"
    assert len(k_fwd_on) == 1 and "mhatt_fwd_kernel" in k_fwd_on[0], k_fwd_on
    assert 1 <= len(k_bwd_on) <= 2 and all("mhatt_bwd_" in n for n in k_bwd_on), k_bwd_on
    assert len(k_fwd_on) < len(k_fwd_off) and len(k_bwd_on) < len(k_bwd_off)


def test_the_module_takes_the_route_only_when_eligible(dev, att_on):
    """with the switch on: device fp32 tensors of an eligible size launch the kernels; a per-query mask, a head size of 48 and
    fp64 do not, and give the composition's bits"""
    from bridgeqa_amd import _ext
    torch.manual_seed(9)
    B, Nq, Nk = 2, 5, 9
    att = att_on.MHAtt(64, num_heads=2, pdrop=0.0).to(dev)
    x, y = torch.randn(B, Nq, 64, device=dev), torch.randn(B, Nk, 64, device=dev)
    calls = list(_ext.MHATT_CALLS)
    out = att(y, y, x, None)
    assert [a - b for a, b in zip(_ext.MHATT_CALLS, calls)] == [1, 0]
    assert (out - R.composition_mhatt(att, y, y, x, None)).abs().max() < 1e-4
    calls = list(_ext.MHATT_CALLS)
    full = torch.zeros(B, 1, Nq, Nk, dtype=torch.bool, device=dev)
    full[:, :, ::2, 1] = True
    assert torch.equal(att(y, y, x, full), R.composition_mhatt(att, y, y, x, full))
    att96 = att_on.MHAtt(96, num_heads=2, pdrop=0.0).to(dev)
    x96 = torch.randn(B, Nq, 96, device=dev)
    assert torch.equal(att96(x96, x96, x96, None), R.composition_mhatt(att96, x96, x96, x96, None))
    att64 = copy.deepcopy(att).double()
    assert torch.equal(att64(y.double(), y.double(), x.double(), None), R.composition_mhatt(att64, y.double(), y.double(), x.double(), None))
    assert _ext.MHATT_CALLS == calls


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_eval_forward_and_backward_replay_from_one_graph(dev, att_on):
    """An attention site in eval mode (keep = None; what MHAtt.forward runs between the three linears and linear_merge): forward
    + backward captured on one stream (no fork) and replayed twice is bitwise the eager result.  The eager pass runs on the
    stream of the capture, as in tests/test_mcan_rows_gpu.py: autograd nodes remember the stream they were born on."""
    from bridgeqa_amd import _ext
    d = R.inputs((3, 8, 37, 9, 32), "mixed", False)
    heads = d["heads"]
    q, k, v = [t.requires_grad_(True) for t in _to(dev, d["q"], d["k"], d["v"])]
    dy = d["dout"].to(dev)
    hide8 = d["hide"].to(dev).view(torch.uint8)
    leaves = (q, k, v)

    def fwd_bwd():
        out = att_on._MHAttCoreFn.apply(q, k, v, hide8, None, heads)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, dy))
    calls = list(_ext.MHATT_CALLS)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eager = [t.clone() for t in fwd_bwd()]
    torch.cuda.synchronize(dev)
    assert [a - b for a, b in zip(_ext.MHATT_CALLS, calls)] == [1, 1]
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
