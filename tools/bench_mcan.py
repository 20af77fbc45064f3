"""Times the MCAN blocks with the fused row kernels of csrc/mcan.hip (mcan_module.set_fused(True): residual LayerNorm and AttFlat's
pooling, one kernel each way) against the torch compositions, and as a third route with the attention kernels of csrc/mhatt.hip
on top of the row kernels (mcan_module.set_fused_attention(True): MHAtt's core, one launch forward and two backward per site),
same weights, inputs and seed, forward + loss + backward:

  * the stage-1 question branch (hotpath.lang_branch_forward: LangModule, MCAN_ED with 2 + 2 layers, two AttFlat heads,
    fusion_norm, the three classifiers) at B in {16, 64} x question length in {14, 32}, 256 proposals, hidden 256;
  * the VQA reference head (hotpath.qa_heads_forward with use_reference: dec_list_qo, 2 SGA layers over 256 proposals against
    the question states) at the same sizes.

HIP events around blocks of calls, warm-up of every shape, the three routes alternated in the same process, the median over the
blocks; device kernels per call from one call under torch.profiler (a run of its own, after the timing).  The tables of
profiles/mcan_rows.md (two routes) and profiles/mhatt.md (three) are this tool's output.

    python tools/bench_mcan.py [--blocks 7] [--calls 20] [--warmup 5] [--out OUT.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lstm import alternate, kernels  # noqa: E402  (the timing and kernel-count helpers, shared)

SIZES = [(16, 14), (16, 32), (64, 14), (64, 32)]      # (B, question length)
K, HID, EMB, BLIP = 256, 256, 300, 768


def with_route(fused, fn, attention=False):
    def run():
        from bridgeqa_amd import mcan_module
        prev, prev_att = mcan_module.set_fused(fused), mcan_module.set_fused_attention(attention)
        try:
            return fn()
        finally:
            mcan_module.set_fused(prev)
            mcan_module.set_fused_attention(prev_att)
    return run


def _batch(B, L, dev):
    import torch
    g = torch.Generator().manual_seed(100 * B + L)
    lens = torch.randint(3, L + 1, (B,), generator=g)
    lens[0] = L
    n_obj = torch.randint(K // 4, K + 1, (B,), generator=g)
    object_mask = (torch.arange(K)[None, :] >= n_obj[:, None]).view(B, 1, 1, K).to(dev)      # True = NOT an object
    return dict(lang_feat=torch.randn(B, L, EMB, generator=g).to(dev), lang_len=lens,
                objectness_scores=torch.randn(B, K, 2, generator=g).to(dev),
                object_feat=torch.randn(B, K, HID, generator=g).to(dev).requires_grad_(True), object_mask=object_mask,
                fused_feat=torch.randn(B, L, BLIP, generator=g).to(dev),
                fused_mask=(torch.arange(L)[None, :] < lens[:, None]).long().to(dev), gen=g)


def _step(module, forward, weights):
    """forward + loss (a fixed random functional of every output) + backward; returns the outputs"""
    import torch

    def run():
        torch.manual_seed(0)                      # the same dropout masks on either route
        for p in module.parameters():
            p.grad = None
        out = forward()
        loss = sum((out[k] * w).sum() for k, w in weights.items())
        loss.backward()
        return out
    return run


def _compare(fn, module, keys, attention=False):
    """largest |difference| of the outputs, and of the parameter gradients relative to the largest gradient entry, between the
    fused route (with the attention kernels too when `attention`) and the compositions (one scale for all tensors: the
    key-projection biases have a gradient of exactly zero in real arithmetic, rounding noise on either route, and would make a
    per-tensor ratio meaningless)"""
    out_on = with_route(True, fn, attention)()
    g_on = [p.grad.clone() for p in module.parameters() if p.grad is not None]
    out_off = with_route(False, fn)()
    g_off = [p.grad for p in module.parameters() if p.grad is not None]
    d_out = max(float((out_on[k] - out_off[k]).detach().abs().max()) for k in keys)
    d_grad = max(float((a - b).abs().max()) for a, b in zip(g_on, g_off)) / max(float(b.abs().max()) for b in g_off)
    return d_out, d_grad


def bench(a, dev):
    import torch
    import torch.nn as nn
    from bridgeqa_amd import _ext, hotpath
    torch.manual_seed(0)
    branch = hotpath.build_lang_branch(nn.Module(), HID, 18, 8864).to(dev).train()
    heads = hotpath.build_qa_heads(nn.Module(), HID, BLIP, 18).to(dev).train()
    res = {}
    for B, L in SIZES:
        b = _batch(B, L, dev)
        g = b["gen"]
        w_branch = dict(lang_scores=torch.randn(B, 18, generator=g).to(dev), answer_scores=torch.randn(B, 8864, generator=g).to(dev),
                        cluster_ref=torch.randn(B, K, generator=g).to(dev))
        w_heads = dict(cluster_ref=torch.randn(B, K, generator=g).to(dev))
        fns = {
            "branch": (branch, _step(branch, lambda: hotpath.lang_branch_forward(
                branch, dict(lang_feat=b["lang_feat"], lang_len=b["lang_len"], objectness_scores=b["objectness_scores"]),
                b["object_feat"], b["object_mask"], True, True, True), w_branch), w_branch),
            "vqa_ref_head": (heads, _step(heads, lambda: hotpath.qa_heads_forward(
                heads, dict(objectness_scores=b["objectness_scores"]), b["object_feat"], b["object_mask"], b["fused_feat"],
                b["fused_mask"], False, True), w_heads), w_heads),
        }
        for name, (module, fn, weights) in fns.items():
            c0 = list(_ext.MCAN_CALLS)
            d_out, d_grad = _compare(fn, module, list(weights))
            took = [p - q for p, q in zip(_ext.MCAN_CALLS, c0)]
            want = [11, 11, 2, 2] if name == "branch" else [6, 6, 0, 0]
            assert took == want, "%s: the fused variant launched %s, expected %s" % (name, took, want)
            c0, h0 = list(_ext.MCAN_CALLS), list(_ext.MHATT_CALLS)
            d_out_att, d_grad_att = _compare(fn, module, list(weights), attention=True)
            assert [p - q for p, q in zip(_ext.MCAN_CALLS, c0)] == want, "%s: the attention route changed the row launches" % name
            took = [p - q for p, q in zip(_ext.MHATT_CALLS, h0)]
            want = [6, 6] if name == "branch" else [4, 4]
            assert took == want, "%s: the attention variant launched %s attention sites, expected %s" % (name, took, want)
            routes = {"fused": with_route(True, fn), "composition": with_route(False, fn), "fused_att": with_route(True, fn, True)}
            t = alternate(routes, a.warmup, a.blocks, a.calls)
            row = dict(t, kernels={k: kernels(r) for k, r in routes.items()}, max_abs_diff_out=d_out, max_rel_diff_grad=d_grad,
                       max_abs_diff_out_att=d_out_att, max_rel_diff_grad_att=d_grad_att)
            res["%s_B%d_L%d" % (name, B, L)] = row
            print("%-12s B %2d L %2d  fwd+bwd fused %7.3f ms (min %7.3f max %7.3f)  composition %7.3f ms (min %7.3f max %7.3f)  "
                  "fused + attention %7.3f ms (min %7.3f max %7.3f) | kernels %d vs %d vs %d | max |diff| to the composition: "
                  "out %.2g, grads (of the largest) %.2g; with attention %.2g, %.2g" % (
                      name, B, L, t["fused"]["median_ms"], t["fused"]["min_ms"], t["fused"]["max_ms"],
                      t["composition"]["median_ms"], t["composition"]["min_ms"], t["composition"]["max_ms"],
                      t["fused_att"]["median_ms"], t["fused_att"]["min_ms"], t["fused_att"]["max_ms"],
                      row["kernels"]["fused"], row["kernels"]["composition"], row["kernels"]["fused_att"], d_out, d_grad,
                      d_out_att, d_grad_att), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcan.py: no GPU visible (a measurement path does not fall back)")
    dev = torch.device("cuda:0")
    res = {"K": K, "hidden": HID, "blocks": a.blocks, "calls": a.calls, "rows": bench(a, dev)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
