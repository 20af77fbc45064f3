"""Times the question branch's LSTM (lang_module.LangModule, E = 300, H = 256, one layer, one direction: ScanQA's defaults) on
the device, forward + backward, on the fused route (csrc/lstm.hip) against the held nn.LSTM on packed input (the vendor RNN
library), same weights and inputs: B in {16, 64} x question length in {14, 32} (ragged lengths, the longest = the length).
Then one eager DET-stage step (forward + loss + backward, bf16 detector path, c2 sizes: 16 scenes x 40000 points x 132
channels) without the branch, and with it on either LSTM route.

HIP events around blocks of calls, warm-up of every shape, the two routes alternated in the same process, the median over the
blocks; device kernels per call from one call under torch.profiler.  The profiles/lang_branch.md table is this tool's output.

    python tools/bench_lstm.py [--blocks 7] [--calls 20] [--warmup 5] [--no-step] [--out OUT.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(16, 14), (16, 32), (64, 14), (64, 32)]      # (B, question length)
E, H = 300, 256


def block_ms(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, warmup, blocks, calls):
    """{name: median ms per call}; every block times each variant once, in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            times[k].append(block_ms(fn, calls))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return len([n for n in names if "emcpy" not in n and "emset" not in n])


def with_route(fused, fn):
    def run():
        os.environ["BQ_LSTM_FUSED"] = "1" if fused else "0"
        return fn()
    return run


def bench_lstm(a, dev):
    import torch
    from bridgeqa_amd import _ext
    from bridgeqa_amd.lang_module import LangModule
    torch.manual_seed(0)
    m = LangModule(18, use_lang_classifier=False, emb_size=E, hidden_size=H, pdrop=0.0).to(dev).train()
    res = {}
    for B, L in SIZES:
        g = torch.Generator().manual_seed(100 * B + L)
        x = torch.randn(B, L, E, generator=g).to(dev).requires_grad_(True)
        lens = torch.randint(3, L + 1, (B,), generator=g)
        lens[0] = L
        g_out, g_emb = torch.randn(B, L, H, generator=g).to(dev), torch.randn(B, H, generator=g).to(dev)

        def fwd():
            return m({"lang_feat": x, "lang_len": lens})

        def fwd_bwd():
            d = fwd()
            for p in m.parameters():
                p.grad = None
            x.grad = None
            ((d["lang_out"] * g_out).sum() + (d["lang_emb"] * g_emb).sum()).backward()
            return d
        c0 = list(_ext.LSTM_CALLS)
        d_f = with_route(True, fwd_bwd)()
        assert [p - q for p, q in zip(_ext.LSTM_CALLS, c0)] == [1, 1], "the fused variant did not take its route"
        gf = [p.grad.clone() for p in m.parameters()]
        d_l = with_route(False, fwd_bwd)()
        assert [p - q for p, q in zip(_ext.LSTM_CALLS, c0)] == [1, 1], "the nn.LSTM variant launched the fused kernels"
        diff = dict(out=float((d_f["lang_out"] - d_l["lang_out"]).abs().max()),
                    grad=max(float((p.grad - q).abs().max() / q.abs().max()) for p, q in zip(m.parameters(), gf)))
        t = alternate({"fused": with_route(True, fwd_bwd), "nn_lstm": with_route(False, fwd_bwd),
                       "fused_fwd": with_route(True, fwd), "nn_lstm_fwd": with_route(False, fwd)}, a.warmup, a.blocks, a.calls)
        row = dict(t, kernels=dict(fused=kernels(with_route(True, fwd_bwd)), nn_lstm=kernels(with_route(False, fwd_bwd))),
                   max_abs_diff_out=diff["out"], max_rel_diff_grad=diff["grad"])
        res["B%d_L%d" % (B, L)] = row
        print("B %2d L %2d  fwd+bwd fused %7.3f ms  nn.LSTM %7.3f ms | fwd fused %7.3f ms  nn.LSTM %7.3f ms | kernels %d vs %d | "
              "max |diff| out %.2g, grads (rel) %.2g" % (B, L, t["fused"]["median_ms"], t["nn_lstm"]["median_ms"],
                                                         t["fused_fwd"]["median_ms"], t["nn_lstm_fwd"]["median_ms"],
                                                         row["kernels"]["fused"], row["kernels"]["nn_lstm"], diff["out"],
                                                         diff["grad"]), flush=True)
    w = m.lstm.weight_hh_l0
    res["w_hh_transpose_ms"] = alternate({"t": lambda: w.t().contiguous()}, a.warmup, a.blocks, 5 * a.calls)["t"]["median_ms"]
    print("W_hh^T (1024 x 256 -> 256 x 1024) per call: %.4f ms" % res["w_hh_transpose_ms"], flush=True)
    return res


def bench_step(a, dev):
    """one eager DET step at c2 sizes: forward + loss + backward (no optimizer), bf16 detector path"""
    import torch
    import bench
    from bridgeqa_amd import fusion_ops
    from bridgeqa_amd.hotpath import ScanQAHotPath
    from bridgeqa_amd.loss_helper import compute_lang_classification_loss

    class A(object):
        points, cin, image = 40000, 132, 512
    B, L = 16, 14
    fusion_ops.set_compute_dtype(torch.bfloat16)
    batch = bench.make_batch(A, "c2", B, 42, dev)
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(3, L + 1, (B,), generator=g)
    lens[0] = L
    batch.update(lang_feat=torch.randn(B, L, E, generator=g).to(dev), lang_len=lens,
                 object_cat=torch.randint(0, 18, (B,), generator=g).to(dev), ref_obj_mask=torch.ones(B, device=dev))
    torch.manual_seed(0)
    plain = ScanQAHotPath(input_feature_dim=A.cin, use_blip=False).to(dev).train()
    torch.manual_seed(0)
    full = ScanQAHotPath(input_feature_dim=A.cin, use_blip=False, lang_branch=True, num_answers=8864, use_lang_cls=True,
                         use_object_mask=True).to(dev).train()

    def step(model, lang):
        def run():
            for p in model.parameters():
                p.grad = None
            out = model(dict(batch))
            loss = bench.det_loss(out)
            if lang:
                loss = loss + compute_lang_classification_loss(out)
            loss.backward()
            return loss
        return run
    fns = {"det_only": step(plain, False), "with_branch_fused": with_route(True, step(full, True)),
           "with_branch_nn_lstm": with_route(False, step(full, True))}
    t = alternate(fns, max(2, a.warmup // 2), a.blocks, max(2, a.calls // 5))
    res = dict(t, kernels={k: kernels(fn) for k, fn in fns.items()})
    for k in fns:
        print("eager DET step (B 16, 40000 points) %-20s median %8.3f ms (min %8.3f, max %8.3f)  kernels %d" % (
            k, t[k]["median_ms"], t[k]["min_ms"], t[k]["max_ms"], res["kernels"][k]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="leave out the eager DET step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm.py: no GPU visible (a measurement path does not fall back)")
    dev = torch.device("cuda:0")
    res = {"E": E, "H": H, "blocks": a.blocks, "calls": a.calls, "lstm": bench_lstm(a, dev)}
    if not a.no_step:
        res["det_step"] = bench_step(a, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
