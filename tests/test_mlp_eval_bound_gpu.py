"""The eval-mode SharedMLP kernel (csrc/mlp_eval.hip, _ext.mlp_eval: every launch of the eval-mode detector) held to exact
results and to the per-element fp64 bound of tests/mlp_eval_ref.py, where tests/test_mlp_eval_gpu.py accepts whole-tensor
norms: one wrong element of a ragged last tile, a tail column beyond 256, a row of a tile that straddles two scenes or a dropped
k-step of one channel tile fails here.

  single layers   rows and grouped form (unpooled and pooled), exact tier (== on values) and bound tier
  tail            the fp32 linear tail against the fp64 tail of the kernel's own stored layer output
  probes          identity / selection layers: the staged input tile (both gathers, coordinates, zero padding, row copies)
                  element for element against RNE_bf16 of the fp32 CPU composition and against _ext.group_concat_pm
  chains          a fused 2- or 3-layer launch EQUALS the layers launched one at a time through HBM rows; pooled EQUALS the
                  max over S of the unpooled launch -- no tolerance
  guard           nothing is written outside the output; R = 0 launches nothing
  route           every _ext.mlp_eval call of one eval-mode bf16 model.detect, recorded: its specs are the fp64 fold of the
                  owning module's conv and BatchNorm tensors, its first layer is inside the bound, fused equals chained

Every case moves the results to the CPU and compares every element; `not (err <= tol)` fails, so NaN fails.  The cases and the
edge each reaches are listed in tests/mlp_eval_ref.py; tests/test_mlp_eval_bound_cpu.py has checked the reference's conditions
on all of them.  The largest |err| / tol per form is printed at the end of the module (pytest -s); on an MI355X:
profiles/mlp_eval_bound.md.
"""
import ctypes
import time

import pytest
import torch

import mlp_eval_ref as M

pytestmark = pytest.mark.gpu

_WORST = {}
_KERNEL = "mlp_eval_kernel"


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print("\nmlp_eval battery: %.1f s; largest |err| / tol per form: %s" % (
        time.time() - t0, "  ".join("%s %.3g" % kv for kv in sorted(_WORST.items()))))


@pytest.fixture(scope="module")
def ext(dev):
    from bridgeqa_amd import _ext
    return _ext


def _dev_spec(spec, dev):
    return None if spec is None else {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in spec.items()}


def _dev_inputs(dev, grouped=None, rows=None):
    """the launch's input keywords on the device; the features are the strided slice of the interleaved cloud"""
    if grouped is not None:
        C = grouped["C"]
        cloud = grouped["cloud"].to(dev)
        return dict(grouped=(grouped["xyz"].to(dev), grouped["new_xyz"].to(dev), cloud[..., 3:3 + C] if C else None,
                             grouped["idx"].to(dev), grouped["radius"], grouped["normalize"]))
    return dict(rows=(rows[0].to(dev), rows[1]))


@pytest.fixture(scope="module")
def launch(ext, dev):
    """_ext.mlp_eval on CPU tensors, the result back on the CPU: what the hold_* functions of the reference call"""
    def run(layers, tail=None, grouped=None, rows=None, pool=False):
        out = ext.mlp_eval([_dev_spec(l, dev) for l in layers], tail=_dev_spec(tail, dev), pool=pool,
                           **_dev_inputs(dev, grouped, rows))
        return out.cpu()
    return run


@pytest.mark.parametrize("c", M.ROWS_CASES, ids=M.case_id)
def test_rows_single_layer(launch, c):
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_single(c, launch, hold)
    hold.assert_ok()


@pytest.mark.parametrize("c", M.GROUPED_CASES, ids=M.case_id)
def test_grouped_single_layer(launch, c):
    """unpooled and pooled; the pooled output also equals the max over S of the unpooled one"""
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_single(c, launch, hold)
    hold.assert_ok()


@pytest.mark.parametrize("c", M.TAIL_CASES, ids=M.case_id)
def test_tail(launch, c):
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_tail(c, launch, hold)
    hold.assert_ok()


@pytest.mark.parametrize("c", M.PROBE_CASES, ids=M.case_id)
def test_staged_tile_probe(launch, ext, dev, c):
    hold = M.Hold(M.case_id(c), _WORST)
    x = M.hold_probe(c, launch, hold)
    if "C" in c and c["C"] <= 256:
        _, K, kw = M.case_rows(c)
        pm = ext.group_concat_pm(*_dev_inputs(dev, **kw)["grouped"], torch.bfloat16)
        hold.equal("staged tile against group_concat_pm", pm.reshape(-1, K).cpu(), x[:, :K])
    hold.assert_ok()


@pytest.mark.parametrize("c", M.CHAIN_CASES, ids=M.case_id)
def test_fused_equals_chained(launch, c):
    hold = M.Hold(M.case_id(c), _WORST)
    M.hold_chain(c, launch, hold)
    hold.assert_ok()


# ---- the output guard -----------------------------------------------------------------------------------------------------------
def _direct(ext, dev, out_ptr, layers, tail=None, grouped=None, rows=None, pool=False):
    """bq_mlp_eval with the descriptor _ext.mlp_eval builds, but the output where the test says"""
    d = ext._MlpEvalDesc()
    if grouped is not None:
        xyz, new_xyz, feats, idx, radius, normalize = grouped
        B, N, _ = xyz.shape
        _, Mm, S = idx.shape
        d.xyz, d.new_xyz, d.idx = xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr()
        d.B, d.N, d.M, d.S, d.radius, d.normalize = B, N, Mm, S, float(radius), int(bool(normalize))
        d.feats, d.C, d.f_bs, d.f_rs = feats.data_ptr(), feats.shape[2], feats.stride(0), feats.stride(1)
        d.R = B * Mm * S
    else:
        x, K = rows
        d.x, d.ldx, d.K, d.R = x.data_ptr(), x.stride(0), int(K), x.shape[0]
    d.n_layers = len(layers)
    for i, spec in enumerate(layers):
        ext._mlp_eval_layer(d.layers[i], spec)
    if tail is not None:
        d.has_tail = 1
        ext._mlp_eval_layer(d.tail, dict(tail, relu=False))
    d.out, d.pool = out_ptr, int(bool(pool))
    with torch.cuda.device(dev):
        ext._check(ext._lib.bq_mlp_eval(ctypes.byref(d), ext._stream()), "mlp_eval")
    torch.cuda.synchronize()


_GUARD_ROWS = dict(id=5000, tier="bound", R=301, K=40)
_GUARD_GROUPED = dict(id=5001, tier="bound", B=2, M=37, S=16, C=132, N=173, radius=0.2, normalize=True)


@pytest.mark.parametrize("form", ("plain", "pooled", "tail"))
def test_nothing_is_written_outside_the_output(ext, dev, form):
    """one direct launch per epilogue into the middle of a sentinel-filled buffer, R no multiple of 64, tail n = 259"""
    c = _GUARD_GROUPED if form == "pooled" else _GUARD_ROWS
    x, K, kw = M.case_rows(c)
    layers = [_dev_spec(M.layer_spec(c["id"], K, 96, "bound"), dev)]
    tail = _dev_spec(M.tail_spec(c["id"], 96, 259), dev) if form == "tail" else None
    kwd = _dev_inputs(dev, **kw)
    want = ext.mlp_eval(layers, tail=tail, pool=form == "pooled", **kwd)
    assert x.shape[0] % M.TM != 0
    pad = 1024
    buf = torch.full((pad + want.numel() + pad,), -1234.5, dtype=want.dtype, device=dev)
    sentinel = buf[:1].clone()
    _direct(ext, dev, buf.data_ptr() + pad * buf.element_size(), layers, tail, pool=form == "pooled", **kwd)
    bits = torch.int16 if want.dtype == torch.bfloat16 else torch.int32
    got = buf.cpu().view(bits)
    s = int(sentinel.cpu().view(bits))
    assert bool((got[:pad] == s).all()), "written before the output"
    assert bool((got[pad + want.numel():] == s).all()), "written behind the output"
    assert torch.equal(got[pad:pad + want.numel()], want.cpu().reshape(-1).view(bits))


def test_no_rows_no_launch(ext, dev):
    from torch.profiler import ProfilerActivity, profile
    spec = _dev_spec(M.layer_spec(5002, 40, 96, "bound"), dev)
    tail = _dev_spec(M.tail_spec(5002, 96, 259), dev)
    x = torch.empty(0, 40, dtype=torch.bfloat16, device=dev)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        a = ext.mlp_eval([spec], rows=(x, 40))
        b = ext.mlp_eval([spec], tail=tail, rows=(x, 40))
        torch.cuda.synchronize()
    assert a.shape == (0, 96) and a.dtype == torch.bfloat16 and b.shape == (0, 259) and b.dtype == torch.float32
    assert not [e.name for e in prof.events() if _KERNEL in e.name]


# ---- the route ------------------------------------------------------------------------------------------------------------------
def _owners(model):
    """id(running_mean) -> (conv, bn, relu) of every conv -> BatchNorm pair the eval route folds; id(weight) -> conv of the tails"""
    bb, vote, prop = model.detection_backbone, model.voting_net, model.proposal_net
    pairs, tails = {}, {}
    mlps = [getattr(bb, "sa%d" % i).mlp_module for i in (1, 2, 3, 4)] + [bb.fp1.mlp, bb.fp2.mlp, prop.vote_aggregation.mlp_module]
    for mlp in mlps:
        for l in mlp:
            pairs[id(l.bn.bn.running_mean)] = (l.conv, l.bn.bn, hasattr(l, "activation"))
    for conv, bn in ((vote.conv1, vote.bn1), (vote.conv2, vote.bn2), (prop.proposal[0], prop.proposal[1]),
                     (prop.proposal[3], prop.proposal[4])):
        pairs[id(bn.running_mean)] = (conv, bn, True)
    for conv in (vote.conv3, prop.proposal[6]):
        tails[id(conv.bias)] = conv
    return pairs, tails


def _cpu_spec(spec):
    return None if spec is None else {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in spec.items() if v is not None}


def test_the_route_of_eval_detect(ext, dev, monkeypatch):
    from conftest import scene
    from bridgeqa_amd import fusion_ops
    from bridgeqa_amd.hotpath import ScanQAHotPath
    torch.manual_seed(0)
    model = ScanQAHotPath(input_feature_dim=1, use_blip=False).to(dev).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in model.modules():        # BatchNorm state far from (1, 0, 0, 1), conv biases far from 0
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                n = m.num_features
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=g) * 2 + 0.5)
    pc = scene(1, 2048, 1, seed=7, room=(3.0, 3.0, 1.5)).to(dev)        # 2048 points: SA1 keeps them all
    calls = []
    real = ext.mlp_eval

    def recording(layers, tail=None, grouped=None, rows=None, pool=False):
        out = real(layers, tail=tail, grouped=grouped, rows=rows, pool=pool)
        calls.append((layers, tail, grouped, rows, pool, out))
        return out
    monkeypatch.setattr(ext, "mlp_eval", recording)
    prev = fusion_ops.set_compute_dtype(torch.bfloat16)
    try:
        with torch.no_grad():
            model.detect({"point_clouds": pc})
    finally:
        fusion_ops.set_compute_dtype(prev)
        monkeypatch.setattr(ext, "mlp_eval", real)
    assert len(calls) == 9
    assert [len(c[0]) for c in calls] == [3, 3, 3, 3, 2, 2, 2, 3, 2]
    assert [c[4] for c in calls] == [True] * 4 + [False] * 3 + [True, False]
    assert [c[1] is not None for c in calls] == [False] * 6 + [True, False, True]
    pairs, tails = _owners(model)
    hold = M.Hold("route", _WORST)
    for ci, (layers, tail, grouped, rows, pool, out) in enumerate(calls):
        # ---- the specs are the owning module's tensors
        k = 3 + (grouped[2].shape[2] if grouped[2] is not None else 0) if grouped is not None else rows[1]
        for li, spec in enumerate(layers):
            conv, bn, relu = pairs[id(spec["mean"])]
            cpu = _cpu_spec(spec)
            own = dict(w=cpu["w"], mean=bn.running_mean.cpu(), var=bn.running_var.cpu(), eps=bn.eps, gamma=bn.weight.detach().cpu(),
                       beta=bn.bias.detach().cpu(), relu=relu)
            if conv.bias is not None:
                own["bias"] = conv.bias.detach().cpu()
            for a, b, what in zip(M.fold(cpu)[:2], M.fold(own)[:2], ("s", "t")):
                hold.equal("call %d layer %d %s against the module's fold" % (ci, li, what), a, b)
            hold.true(bool(spec["relu"]) == relu and float(spec["eps"]) == bn.eps, "call %d layer %d: relu / eps" % (ci, li))
            hold.true((spec.get("bias") is None) == (conv.bias is None), "call %d layer %d: bias" % (ci, li))
            w = conv.weight.detach().reshape(conv.out_channels, -1)
            hold.true(w.shape[1] == k, "call %d layer %d: %d inputs against %d" % (ci, li, w.shape[1], k))
            hold.equal("call %d layer %d weight" % (ci, li), cpu["w"][:, :k], w.to(torch.bfloat16).cpu())
            hold.true(bool((cpu["w"][:, k:] == 0).all()), "call %d layer %d: weight padding not zero" % (ci, li))
            k = conv.out_channels
        if tail is not None:
            conv = tails[id(tail["bias"])]
            w = conv.weight.detach().reshape(conv.out_channels, -1)
            hold.equal("call %d tail weight" % ci, tail["w"][:, :k].cpu(), w.to(torch.bfloat16).cpu())
            hold.true(bool((tail["w"][:, k:] == 0).all()), "call %d: tail padding not zero" % ci)
        # ---- fused equals chained, on the recorded operands
        kw = dict(grouped=grouped) if grouped is not None else dict(rows=rows)
        S = grouped[3].shape[2] if grouped is not None else 0
        hold.equal("call %d fused against chained" % ci, out, M.chained(real, layers, tail, kw, S if pool else 0))
        # ---- the first layer inside the single-layer bound
        if grouped is not None:
            xyz, new_xyz, feats, idx, radius, normalize = grouped
            C = feats.shape[2] if feats is not None else 0
            cloud = torch.cat([xyz, feats if feats is not None else xyz[..., :0], xyz[..., :2]], -1).cpu()
            x = M.group_rows(dict(xyz=xyz.cpu(), new_xyz=new_xyz.cpu(), cloud=cloud, C=C, idx=idx.cpu(), radius=radius,
                                  normalize=normalize))
        else:
            x = torch.zeros(rows[0].shape[0], M.ceil32(rows[1]), dtype=torch.bfloat16)
            x[:, :rows[1]] = rows[0][:, :rows[1]].cpu()
        first = real(layers[:1], **kw)
        r, tol = M.layer(x, _cpu_spec(layers[0]))
        hold("route first layer", first, r, tol)
    hold.assert_ok()
