"""The stage-1 question branch on the device: hotpath.lang_branch_forward (LangModule on the fused LSTM route, MCAN_ED, AttFlat,
heads) against the same function on the CPU fallback with identical inputs and weights -- outputs and every parameter's
gradient -- and one ScanQAHotPath(lang_branch=True) forward + lang_loss backward.

Tolerance of the device-vs-CPU comparison (both fp32 evaluations of one function, different summation orders and exp / tanh /
erf routines): 1e-4 of the scale of the quantity.  One 512-term reduction (the FFN's contraction at hidden 128) has a worst-case
rounding error of 512 * 2^-24 = 3e-5 of its terms' magnitude; the branch chains three per layer, and LayerNorm renormalises in
between, so 1e-4 is the worst case of a layer and far above the expected sqrt(n) behaviour.  The scale is the tensor's own
largest magnitude for outputs; for a gradient it is at least the largest gradient magnitude of any parameter, because some
gradients are sums that cancel analytically (the key projection's bias under softmax) and hold rounding noise only."""
import pytest
import torch

from golden_util import fill_params

pytestmark = pytest.mark.gpu

REL = 1e-4
OUT_KEYS = ("lang_out", "lang_emb", "fuse_feat", "lang_scores", "cluster_ref", "answer_scores")


def _run(holder, inp, cot, device):
    from bridgeqa_amd import hotpath
    holder = holder.to(device)
    for p in holder.parameters():
        p.grad = None
    d = {k: v.to(device) for k, v in inp.items()}
    d["lang_len"] = inp["lang_len"]          # the loader delivers the lengths on the host
    object_mask = (~d["bbox_mask"].bool()).unsqueeze(1).unsqueeze(2)
    d = hotpath.lang_branch_forward(holder, d, d["object_feat"], object_mask, True, True, True)
    sum((d[k] * cot[k].to(device)).sum() for k in OUT_KEYS).backward()
    outs = {k: d[k].detach().cpu() for k in OUT_KEYS + ("lang_mask",)}
    grads = {n: p.grad.detach().cpu() for n, p in holder.named_parameters()}
    return outs, grads


def test_branch_on_device_against_cpu_fallback(dev, golden):
    from bridgeqa_amd import _ext, hotpath
    G = golden("lang_branch.npz")
    holder = torch.nn.Module()
    hotpath.build_lang_branch(holder, 128, 18, 30, mcan_flat_mlp_size=64, mcan_flat_out_size=96, lang_emb_size=20)
    holder.eval()
    fill_params(holder, "branch.")
    inp = {k[6:]: torch.from_numpy(v) for k, v in G.items() if k.startswith("br_in_")}
    assert inp["object_feat"].shape == (3, 16, 128) and G["br_out_lang_scores"].shape == (3, 18)
    g = torch.Generator().manual_seed(5)
    cot = {k: torch.randn(G["br_out_" + k].shape, generator=g) for k in OUT_KEYS}
    before = list(_ext.LSTM_CALLS)
    want_o, want_g = _run(holder, inp, cot, torch.device("cpu"))
    assert _ext.LSTM_CALLS == before
    got_o, got_g = _run(holder, inp, cot, dev)
    assert [a - b for a, b in zip(_ext.LSTM_CALLS, before)] == [1, 1]        # the fused route ran, forward and backward
    holder.to("cpu")
    assert torch.equal(got_o["lang_mask"], want_o["lang_mask"])
    worst = {}
    for k in OUT_KEYS:
        scale = want_o[k].abs().max().item()
        worst[k] = (got_o[k] - want_o[k]).abs().max().item() / scale
    gmax = max(v.abs().max().item() for v in want_g.values())
    assert set(got_g) == set(want_g) and len(want_g) > 100
    for n in want_g:
        worst[n] = (got_g[n] - want_g[n]).abs().max().item() / gmax
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("worst device-vs-CPU errors (fraction of scale):", top)
    assert top[0][1] <= REL, top


def test_hot_path_with_lang_branch_forward_and_lang_loss_backward(dev):
    import bench
    from bridgeqa_amd import _ext, fusion_ops
    from bridgeqa_amd.hotpath import ScanQAHotPath
    from bridgeqa_amd.loss_helper import compute_lang_classification_loss
    torch.manual_seed(0)
    B, T = 2, 14
    model = ScanQAHotPath(input_feature_dim=4, use_blip=False, lang_branch=True, num_answers=30, use_lang_cls=True,
                          use_reference=True, use_answer=True, use_object_mask=True).to(dev).train()
    dd = {"point_clouds": bench.synth_batch(B, 4096, 4, 7, dev), "lang_feat": torch.randn(B, T, 300, device=dev),
          "lang_len": torch.tensor([T, 5]), "object_cat": torch.tensor([3, 11], device=dev),
          "ref_obj_mask": torch.ones(B, device=dev)}
    before = list(_ext.LSTM_CALLS)
    prev = fusion_ops.set_compute_dtype(torch.bfloat16)     # the detector's HIP path, as the DET-stage benchmark runs it
    try:
        out = model(dd)
        loss = compute_lang_classification_loss(out)
        loss.backward()
    finally:
        fusion_ops.set_compute_dtype(prev)
    torch.cuda.synchronize()
    assert [a - b for a, b in zip(_ext.LSTM_CALLS, before)] == [1, 1]        # hidden 256: the fused route
    K = out["object_feat"].shape[1]
    shapes = {"lang_out": (B, T, 256), "lang_emb": (B, 256), "lang_mask": (B, T), "fuse_feat": (B, 1024), "lang_scores": (B, 18),
              "cluster_ref": (B, K), "answer_scores": (B, 30)}
    for k, s in shapes.items():
        assert tuple(out[k].shape) == s, k
        assert out[k].dtype == torch.bool or torch.isfinite(out[k]).all(), k
    assert out["lang_mask"].tolist() == [[False] * T, [t >= 5 for t in range(T)]]
    assert torch.isfinite(loss).item()
    branch = ("object_cls", "lang_net", "lang_feat_linear", "lang_cls", "attflat_visual", "attflat_lang", "answer_cls",
              "fusion_backbone", "fusion_norm")
    # lang_loss reaches every parameter of the branch except the two heads it does not read (cluster_ref, answer_scores)
    for n, p in model.named_parameters():
        if n.split(".")[0] in branch:
            if n.split(".")[0] in ("object_cls", "answer_cls"):
                assert p.grad is None, n
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert any(p.grad is not None for p in model.detection_backbone.parameters())   # and flows on into the detector
