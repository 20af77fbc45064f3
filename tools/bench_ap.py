"""Detection evaluation at the real size: ScanNet val through APCalculator -- 312 scenes x 256 proposals x 18 classes with
per-class proposals (every kept proposal is a detection of every class), about 14 ground-truth boxes per scene -- on seeded
synthetic boxes.  One process on the GPU times

  * compute_metrics on the device (torch sorts, bq_ap_match, bq_ap_curve, one copy) against the repo's own numpy path
    (the yardstick: the same segment algorithm on the host),
  * what a batch of 16 costs on its way into the calculator: a packed step (nothing leaves the device) against the
    hand-over to host lists (one copy, ~70 000 tuples) plus a list step,
  * and, at a reduced size, the largest |AP - literal restatement| (tests/ap_ref.py).

Warm-up, then the median of --runs runs, synchronised before every clock reading.  Prints one JSON line; --out FILE
writes it too.  Usage: python tools/bench_ap.py [--scenes 312] [--runs 10] [--host-runs 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bridgeqa_amd.ap_helper import APCalculator, PackedGroundTruths, PackedPredictions  # noqa: E402

K, K2, C, BATCH = 256, 128, 18, 16


def synth_batch(rng, B, dev):
    n_gt = rng.integers(6, 23, B)                                               # about 14 per scene
    lo = rng.random((B, K2, 3)) * [7.0, 7.0, 2.0]
    gext = np.concatenate([lo, lo + rng.random((B, K2, 3)) * 1.2 + 0.3], -1)
    gvalid = np.arange(K2)[None, :] < n_gt[:, None]
    gcls = rng.integers(0, C, (B, K2))
    # proposals: two thirds sit on a ground-truth box of their scene, jittered; the rest anywhere
    pick = rng.integers(0, n_gt[:, None], (B, K))
    near = np.take_along_axis(gext, pick[:, :, None], 1) + rng.normal(size=(B, K, 6)) * 0.12
    lo = rng.random((B, K, 3)) * [7.0, 7.0, 2.0]
    far = np.concatenate([lo, lo + rng.random((B, K, 3)) * 1.2 + 0.3], -1)
    ext = np.where(rng.random((B, K, 1)) < 0.67, near, far).astype(np.float32).astype(np.float64)
    ext[..., 3:] = np.maximum(ext[..., 3:], ext[..., :3] + 0.05)
    score = (rng.random((B, K, C)) * rng.random((B, K, 1))).astype(np.float32)
    valid = rng.random((B, K)) < 0.8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return PackedPredictions(t(ext), t(score), None, t(valid), C), PackedGroundTruths(t(gext), t(gcls), t(gvalid), C)


def corners_of_extents(e):
    """(n, 6) -> (n, 8, 3) corners whose min / max are the extents"""
    idx = np.array([[i, j + 1, k + 2] for i in (0, 3) for j in (0, 3) for k in (0, 3)])
    return e[:, idx]


def to_lists(pp, pg):
    """the host form of one packed batch, built as parse_predictions / parse_groundtruths build it: one hand-over, then tuples"""
    ext, score, valid = pp.ext.cpu().numpy(), pp.score.cpu().numpy(), pp.valid.cpu().numpy()
    gext, gcls, gvalid = pg.ext.cpu().numpy(), pg.cls.cpu().numpy(), pg.valid.cpu().numpy()
    preds, gts = [], []
    for b in range(ext.shape[0]):
        sel = np.nonzero(valid[b])[0]
        corners = corners_of_extents(ext[b])
        preds.append([(c, corners[k], score[b, k, c]) for c in range(score.shape[2]) for k in sel])
        gc = corners_of_extents(gext[b])
        gts.append([(gcls[b, j].item(), gc[j]) for j in range(gext.shape[1]) if gvalid[b, j]])
    return preds, gts


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=10)
    ap.add_argument("--check-scenes", type=int, default=6)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    batches = [synth_batch(rng, min(BATCH, a.scenes - s), dev) for s in range(0, a.scenes, BATCH)]
    thr = (0.25, 0.5)
    calc = APCalculator(thr)
    for pp, pg in batches:
        calc.step(pp, pg)
    res = dict(scenes=a.scenes, proposals=K, classes=C, thresholds=list(thr), runs=a.runs, host_runs=a.host_runs,
               detection_slots=a.scenes * K * C,
               detections=int(sum(int(pp.valid.sum()) for pp, _ in batches)) * C,
               gt_boxes=int(sum(int(pg.valid.sum()) for _, pg in batches)))
    m_dev = calc.compute_metrics(backend="device")
    res["compute_metrics_device_ms"] = median_ms(lambda: calc.compute_metrics(backend="device"), a.runs, 2)
    m_host = calc.compute_metrics(backend="numpy")
    res["compute_metrics_numpy_ms"] = median_ms(lambda: calc.compute_metrics(backend="numpy"), a.host_runs, 0)
    res["device_equals_numpy_bitwise"] = bool(m_dev == m_host)
    res["mAP"] = {str(t): float(m_dev[t]["mAP"]) for t in thr}
    res["AR"] = {str(t): float(m_dev[t]["AR"]) for t in thr}
    # one batch of 16 on its way into the calculator
    pp, pg = batches[0]
    scratch = APCalculator(thr)
    res["packed_step_ms"] = median_ms(lambda: scratch.step(pp, pg), a.runs, 2)
    scratch.reset()
    res["host_lists_and_step_ms"] = median_ms(lambda: scratch.step(*to_lists(pp, pg)), a.runs, 1)
    # reduced size: against the literal restatement
    import ap_ref
    small = APCalculator(thr)
    n = a.check_scenes
    sp = PackedPredictions(pp.ext[:n], pp.score[:n], None, pp.valid[:n], C)
    sg = PackedGroundTruths(pg.ext[:n], pg.cls[:n], pg.valid[:n], C)
    small.step(sp, sg)
    preds, gts = to_lists(sp, sg)
    got = small.eval_det(backend="device")
    worst = 0.0
    for t in thr:
        _, _, want = ap_ref.eval_all(dict(enumerate(preds)), dict(enumerate(gts)), t)
        worst = max([worst] + [abs(got[t][2][c] - want[c]) for c in want])
    res["check_scenes"], res["check_detections"] = n, sum(len(p) for p in preds)
    res["largest_abs_ap_minus_literal"] = worst
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
