"""Times open-ended decoding (BertLMHeadModel.generate, the `inference="generate"` path of BLIP_VQA3D) at the reference's
shape -- 16 samples x 10 beams, 12 layers, vocabulary 30524, max_length 20, question length 14 and 35 -- on three routes in ONE
process: today's growing cache (BQ_DECODE_CACHE=0), the static cache + decode-attention kernel, and the static cache with the
captured step replayed.  [SEP] is suppressed so that all 19 steps run.  HIP events, warm-up, the median of >= 10 decodes; the
device kernels per decode step of each route come from one decode under torch.profiler.

    python tools/bench_generate.py [--decodes 12] [--warmup 3] [--out OUT.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, BEAMS, MAXLEN = 16, 10, 20
PAD, BOS, SEP = 0, 30522, 102


def make(dev):
    from bridgeqa_amd import med
    cfg = med.BertConfig()     # med_config.json: 12 layers, hidden 768, 12 heads, vocabulary 30524
    torch.manual_seed(0)
    dec = med.BertLMHeadModel(config=cfg).to(dev).eval()
    with torch.no_grad():
        dec.cls.predictions.bias[SEP] = -1e4       # no hypothesis ever finishes: every decode runs max_length - 1 steps
    return dec


def routes():
    from bridgeqa_amd import med

    def setter(cache, graph):
        def f():
            med._DECODE_CACHE[0], med._DECODE_GRAPH[0] = cache, graph
        return f
    return [("today", setter(False, False)), ("cache", setter(True, False)), ("cache+replay", setter(True, True))]


def decode(dec, enc, em, dev):
    bos = torch.full((B, 1), BOS, dtype=torch.long, device=dev)
    return dec.generate(bos, max_length=MAXLEN, min_length=1, num_beams=BEAMS, eos_token_id=SEP, pad_token_id=PAD,
                        encoder_hidden_states=enc, encoder_attention_mask=em)


def kernels_per_decode(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return len([n for n in names if "emcpy" not in n and "emset" not in n]), len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decodes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bridgeqa_amd import fusion_ops as ops
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.bfloat16)
    dec = make(dev)
    res = {"shape": dict(samples=B, beams=BEAMS, layers=12, vocab=30524, max_length=MAXLEN), "decodes": a.decodes, "lq": {}}
    for Lq in (14, 35):
        g = torch.Generator().manual_seed(Lq)
        enc = torch.randn(B * BEAMS, Lq, 768, generator=g).to(dev).to(torch.bfloat16)
        em = torch.ones(B * BEAMS, Lq, dtype=torch.long, device=dev)
        em[BEAMS:2 * BEAMS, Lq // 2:] = 0
        row = {}
        for name, select in routes():
            select()
            for _ in range(a.warmup):
                seq = decode(dec, enc, em, dev)
            assert seq.shape == (B, MAXLEN), seq.shape     # all 19 steps ran
            times = []
            for _ in range(a.decodes):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                decode(dec, enc, em, dev)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            kern, dev_events = kernels_per_decode(lambda: decode(dec, enc, em, dev))
            row[name] = dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                             kernels_per_step=kern / (MAXLEN - 1), device_events_per_step=dev_events / (MAXLEN - 1))
            print("Lq %2d  %-13s median %8.3f ms  (min %8.3f, max %8.3f)  kernels/step %.1f" % (
                Lq, name, row[name]["median_ms"], row[name]["min_ms"], row[name]["max_ms"], row[name]["kernels_per_step"]),
                flush=True)
        res["lq"][str(Lq)] = row
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
