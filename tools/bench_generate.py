"""Times open-ended decoding (BertLMHeadModel.generate, the `inference="generate"` path of BLIP_VQA3D) at the reference's
shape -- 16 samples x 10 beams, 12 layers, vocabulary 30524, max_length 20, question length 14 and 35 -- on four routes in ONE
process: today's growing cache (BQ_DECODE_CACHE=0), the static cache + decode-attention kernel, the static cache with the
captured step replayed (the default), and that with the beam search itself on the device (BQ_BEAM_DEVICE=1: one graph replay
per token).  --mode suppressed: [SEP] is suppressed so that all 19 steps run.  --mode finish: [SEP] is favoured and the LM head
sharpened so that decodes finish early -- what tells whether the device route's lagging stop check costs anything.  HIP events,
warm-up, the median of >= 10 decodes; the device kernels per decode step of each route come from one decode under
torch.profiler; steps run and the host's time inside the step calls (launching, or replaying) from one decode with a timer
around DecodeSession.step / step_beams.

    python tools/bench_generate.py [--mode suppressed|finish] [--sep-bias 8] [--decodes 12] [--warmup 3] [--out OUT.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, BEAMS, MAXLEN = 16, 10, 20
PAD, BOS, SEP = 0, 30522, 102


def make(dev, mode="suppressed", sep_bias=8.0):
    from bridgeqa_amd import med
    cfg = med.BertConfig()     # med_config.json: 12 layers, hidden 768, 12 heads, vocabulary 30524
    torch.manual_seed(0)
    dec = med.BertLMHeadModel(config=cfg).to(dev).eval()
    with torch.no_grad():
        if mode == "suppressed":
            dec.cls.predictions.bias[SEP] = -1e4   # no hypothesis ever finishes: every decode runs max_length - 1 steps
        else:                                      # sharpened as the tests' decoders are, [SEP] favoured: decodes finish early
            dec.cls.predictions.bias.copy_(torch.randn(cfg.vocab_size, device=dev) * 1.5)
            dec.cls.predictions.decoder.weight.mul_(8.0)
            dec.cls.predictions.bias[SEP] += sep_bias
    return dec


def routes():
    from bridgeqa_amd import med

    def setter(cache, graph, beams=False):
        def f():
            med._DECODE_CACHE[0], med._DECODE_GRAPH[0], med._BEAM_DEVICE[0] = cache, graph, beams
        return f
    return [("today", setter(False, False)), ("cache", setter(True, False)), ("cache+replay", setter(True, True)),
            ("device beams", setter(True, True, True))]


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


def host_step_time(fn):
    """(step calls of one decode, host milliseconds spent inside them): DecodeSession.step / step_beams under a timer"""
    from bridgeqa_amd import med
    stat, saved = [0, 0.0], (med.DecodeSession.step, med.DecodeSession.step_beams)

    def timed(orig):
        def f(*a, **k):
            t0 = time.perf_counter()
            out = orig(*a, **k)
            stat[0] += 1
            stat[1] += time.perf_counter() - t0
            return out
        return f
    med.DecodeSession.step, med.DecodeSession.step_beams = timed(saved[0]), timed(saved[1])
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        med.DecodeSession.step, med.DecodeSession.step_beams = saved
    return stat[0], stat[1] * 1e3, wall * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decodes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", choices=("suppressed", "finish"), default="suppressed")
    ap.add_argument("--sep-bias", type=float, default=8.0)
    a = ap.parse_args()
    from bridgeqa_amd import fusion_ops as ops
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.bfloat16)
    dec = make(dev, a.mode, a.sep_bias)
    res = {"mode": a.mode, "shape": dict(samples=B, beams=BEAMS, layers=12, vocab=30524, max_length=MAXLEN), "decodes": a.decodes, "lq": {}}
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
            assert a.mode == "finish" or seq.shape == (B, MAXLEN), seq.shape     # all 19 steps ran
            times = []
            for _ in range(a.decodes):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                decode(dec, enc, em, dev)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            kern, dev_events = kernels_per_decode(lambda: decode(dec, enc, em, dev))
            # (the growing cache has no DecodeSession: its steps are not counted; [SEP] suppressed, every route runs 19)
            steps, in_step_ms, wall_ms = host_step_time(lambda: decode(dec, enc, em, dev))
            n = steps if steps else MAXLEN - 1
            row[name] = dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), steps=steps,
                             kernels_per_step=kern / n, device_events_per_step=dev_events / n,
                             host_ms_in_step_calls_per_step=in_step_ms / n, wall_ms_per_step=wall_ms / n,
                             returned_length=int(seq.shape[1]))
            print("Lq %2d  %-13s median %8.3f ms  (min %8.3f, max %8.3f)  steps %2d  kernels/step %.1f  host in step calls "
                  "%.3f ms/step  wall %.3f ms/step" % (Lq, name, row[name]["median_ms"], row[name]["min_ms"], row[name]["max_ms"],
                                                       steps, row[name]["kernels_per_step"], in_step_ms / n, wall_ms / n), flush=True)
        res["lq"][str(Lq)] = row
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
