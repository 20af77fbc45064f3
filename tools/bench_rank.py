"""Times answer ranking (BLIP_VQA3D.rank_answer, the `inference="rank"` path) at the reference's shape -- 16 questions, 4500
candidate answers, 12 layers, vocabulary 30524 -- with the shared-question route off (question states tiled k times, the
reference's composition) and on (BQ_RANK_SHARED: K/V of the untiled states + csrc/attn_rank.hip), on the same weights and
inputs: k in {128, 256} x question length in {14, 35} x answer length in {6, 12}.  A third variant times the cross form alone
against ops.attention_q_kv (the MFMA kernels) on the (Bq, k * La, H, 64) view of the same queries.

Every variant runs in a fresh child process under its own time limit (the parent never touches the GPU).  HIP events, warm-up,
the median of the timed calls; device kernels per call from one call under torch.profiler; peak memory from the allocator.

    python tools/bench_rank.py [--calls 7] [--warmup 2] [--timeout 420] [--out OUT.json]
"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BQ, N_ANS, H = 16, 4500, 12
PAD, BOS = 0, 30522
SIZES = list(itertools.product((128, 256), (14, 35), (6, 12)))      # (k, Lq, La)
VARIANTS = ("off", "on", "cross")


def inputs(k, Lq, La, dev):
    import torch
    g = torch.Generator().manual_seed(1000 * k + 10 * Lq + La)
    states = torch.randn(BQ, Lq, 768, generator=g).to(dev).to(torch.bfloat16)
    qmask = torch.ones(BQ, Lq, dtype=torch.long)
    for b in range(BQ):
        if b % 5:
            qmask[b, Lq - b % 5:] = 0                               # ragged question lengths
    ids = torch.randint(1000, 30000, (N_ANS, La), generator=g)
    ids[:, 0] = BOS
    lens = torch.randint(2, La + 1, (N_ANS,), generator=g)
    lens[0] = La
    atts = (torch.arange(La)[None, :] < lens[:, None]).long()
    ids = ids * atts
    return states, qmask.to(dev), ids.to(dev), atts.to(dev)


def timed(fn, warmup, calls):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))


def kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return len([n for n in names if "emcpy" not in n and "emset" not in n])


def child_rank(on, a):
    import torch
    from types import SimpleNamespace
    from bridgeqa_amd import _ext, fusion_ops as ops, med
    from bridgeqa_amd.blip_vqa_3d import BLIP_VQA3D
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.bfloat16)
    med._RANK_SHARED[0] = on
    torch.manual_seed(0)
    dec = med.BertLMHeadModel(config=med.BertConfig()).to(dev).eval()
    host = SimpleNamespace(text_decoder=dec, text_decoder_scene=dec, tokenizer=SimpleNamespace(pad_token_id=PAD))
    res = {}
    for k, Lq, La in SIZES:
        states, qmask, ids, atts = inputs(k, Lq, La, dev)

        def call():
            with torch.no_grad():
                return BLIP_VQA3D.rank_answer(host, states, qmask, ids, atts, k)
        calls0 = list(_ext.RANK_CALLS)
        idx, lp = call()
        assert tuple(lp.shape) == (BQ, k) and bool(torch.isfinite(lp).all())
        assert (_ext.RANK_CALLS != calls0) == on, "the variant did not take its route"
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        row = timed(call, a.warmup, a.calls)
        row["peak_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20
        row["kernels_per_call"] = kernels(call)
        row["checksum"] = float(lp.double().sum())
        res["k%d_Lq%d_La%d" % (k, Lq, La)] = row
        print("%-3s k %3d Lq %2d La %2d  median %8.3f ms (min %8.3f, max %8.3f)  kernels %4d  peak %7.0f MB" % (
            "on" if on else "off", k, Lq, La, row["median_ms"], row["min_ms"], row["max_ms"], row["kernels_per_call"],
            row["peak_mb"]), flush=True)
    return res


def child_cross(a):
    """one layer's cross-attention of the re-score: attn_rank_cross (group = k) against the MFMA kernels on the view that makes
    the k * La queries of a question one sequence -- both read the same untiled K/V block"""
    import torch
    from bridgeqa_amd import _ext, fusion_ops as ops
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.bfloat16)
    res = {}
    for k, Lq, La in SIZES:
        g = torch.Generator().manual_seed(k + Lq + La)
        q = (torch.randn(BQ * k, La, H, 64, generator=g)).to(dev).to(torch.bfloat16)
        kv = (torch.randn(BQ, Lq, 2, H, 64, generator=g)).to(dev).to(torch.bfloat16)
        mask = torch.zeros(BQ, 1, 1, Lq, device=dev)
        mask[1, :, :, Lq // 2:] = -1e9
        mlog2 = _ext.key_mask_log2(mask, BQ, Lq)
        qv = q.view(BQ, k * La, H, 64)
        with torch.no_grad():
            r = _ext.attn_rank_cross(q, kv, 0.125, k, mlog2)
            m = ops.attention_q_kv(qv, kv, 0.125, 0.0, mask)
            diff = float((r.float().view_as(m) - m.float()).abs().max())
            t_rank = timed(lambda: _ext.attn_rank_cross(q, kv, 0.125, k, mlog2), a.warmup + 3, 5 * a.calls)
            t_mfma = timed(lambda: ops.attention_q_kv(qv, kv, 0.125, 0.0, mask), a.warmup + 3, 5 * a.calls)
        res["k%d_Lq%d_La%d" % (k, Lq, La)] = dict(rank_cross=t_rank, mfma_view=t_mfma, max_abs_diff=diff)
        print("cross k %3d Lq %2d La %2d  attn_rank_cross %7.3f ms   attention_q_kv on the view %7.3f ms   max |diff| %.3g" % (
            k, Lq, La, t_rank["median_ms"], t_mfma["median_ms"], diff), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per variant")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=VARIANTS)
    ap.add_argument("--result", default=None, help="(child) where to leave the variant's JSON")
    a = ap.parse_args()
    if a.child is not None:
        res = child_cross(a) if a.child == "cross" else child_rank(a.child == "on", a)
        json.dump(res, open(a.result, "w"))
        return 0
    res = {"shape": dict(questions=BQ, candidates=N_ANS, layers=12, vocab=30524), "calls": a.calls, "variants": {}}
    for v in a.variants.split(","):
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "result.json")
            # the child writes its lines straight to this process' stdout; its figures come back through a file
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", v, "--calls", str(a.calls),
                                  "--warmup", str(a.warmup), "--result", out])
            try:
                status = p.wait(timeout=a.timeout)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
                print("variant %s: no result within %d s; stopping" % (v, a.timeout), flush=True)
                return 1
            if status != 0:
                print("variant %s: exit status %d; stopping" % (v, status), flush=True)
                return 1
            res["variants"][v] = json.load(open(out))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
