"""Times training-scene preparation on the device (bridgeqa_amd.scene_data over csrc/scene_prep.hip) at the sizes of the
flagship configurations, and the numpy definition of tests/sceneprep_ref.py on one host core of the same machine.

    python tools/bench_scene_prep.py [--out profiles/scene_prep.json] [--seconds 1.5]

Per size it prints one JSON line:
  kernels_ms        device ms per batch of the three launches alone (parameters already on the device, `out` preallocated):
                    device events around `iters` back-to-back batches after a warm-up, iters chosen so the window exceeds --seconds
  kernels_gbs       algorithmic bytes / kernels_ms.  Algorithmic bytes per sampled point: the gathered row read and written
                    (2 * 4 D), its choice, instance and semantic label (12), vote_label (36) and vote_label_mask (8)
  prepare_ms        device ms per batch of SceneBatcher.prepare(params=None, out=...): the draws (torch.randperm per sample,
                    twelve host numbers per sample), their upload and the three launches
  prepare_host_ms   host wall-clock per batch of the same loop, ended by a device synchronise
  numpy_ms_per_sample  tests/sceneprep_ref.prepare_sample on one core (torch / BLAS threads set to 1), scene already in memory
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIZES = (("c2/c3", 16, 40000, 50000, 135), ("c5", 32, 80000, 100000, 135))
NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


def synth_scene(rs, P, D, n_inst=45, K=30):
    """a scene of ScanNet's shape: P points in runs of n_inst instances, a third of them on non-voting semantics, K boxes"""
    rows = rs.randn(P, D).astype(np.float32)
    rows[:, 0:3] *= np.array([4.0, 4.0, 1.5], dtype=np.float32)
    inst = np.sort(rs.randint(0, n_inst, P))
    sem_of = np.where(np.arange(n_inst) % 3 == 0, 1, NYU40IDS[np.arange(n_inst) % len(NYU40IDS)])
    boxes = np.zeros((K, 8))
    boxes[:, 0:3], boxes[:, 3:6] = rs.uniform(-4, 4, (K, 3)), rs.uniform(0.2, 2.5, (K, 3))
    boxes[:, 6], boxes[:, 7] = NYU40IDS[rs.randint(0, len(NYU40IDS), K)], np.arange(K)
    return dict(rows=rows, instance_labels=inst, semantic_labels=sem_of[inst], instance_bboxes=boxes)


def timed(fn, seconds):
    """-> (device ms per call, host ms per call, calls): warm-up, a probe of 5 calls, then a window longer than `seconds`"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    iters = max(20, int(seconds / max((time.perf_counter() - t0) / 5, 1e-6)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--scenes", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scene_prep: needs a GPU (there is no CPU fallback and no CPU timing)")
    import sceneprep_ref as R
    from bridgeqa_amd import _ext
    from bridgeqa_amd.scene_data import SceneBatcher, SceneStore, draw_params, pack_transform
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    cfg = dict(nyu40ids=NYU40IDS, nyu40id2class={int(v): i for i, v in enumerate(NYU40IDS)},
               mean_size_arr=0.3 + np.random.RandomState(7).rand(len(NYU40IDS), 3))
    results = []
    for name, B, N, P, D in SIZES:
        rs = np.random.RandomState(0)
        scenes = [synth_scene(rs, P, D) for _ in range(args.scenes)]
        store = SceneStore(scenes, dev, **cfg)
        batcher = SceneBatcher(store, N)
        index = [b % len(scenes) for b in range(B)]
        oids = [b % 30 for b in range(B)]
        out = batcher.empty(B)
        params = [draw_params(rs, P, N) for _ in range(B)]
        # the three launches alone
        scene = torch.tensor(index, dtype=torch.int32, device=dev)
        oid = torch.tensor(oids, dtype=torch.int32, device=dev)
        ch = torch.from_numpy(np.stack([p["choices"] for p in params]).astype(np.int32)).to(dev)
        xf = torch.from_numpy(np.stack([pack_transform(p) for p in params])).to(dev)
        table = torch.empty(B, store.max_instance_id + 1, _ext.SCENE_ENTRY, dtype=torch.int32, device=dev)
        k_ms, _, k_iters = timed(lambda: _ext.scene_prep(store, scene, oid, ch, xf, out, table), args.seconds)
        g = torch.Generator(device=dev).manual_seed(0)
        p_ms, p_host_ms, p_iters = timed(lambda: batcher.prepare(index, oids, generator=g, out=out), args.seconds)
        t0, n_ref = time.perf_counter(), 4
        for b in range(n_ref):
            R.prepare_sample(scenes[index[b]], params[b], max_boxes=128, object_id=oids[b], **cfg)
        ref_ms = (time.perf_counter() - t0) * 1e3 / n_ref
        nbytes = B * N * (2 * 4 * D + 12 + 36 + 8)
        res = dict(size=name, B=B, N=N, P=P, D=D, store_mb=round(store.nbytes / 2 ** 20, 1), launches=3,
                   algorithmic_mb=round(nbytes / 1e6, 1), kernels_ms=round(k_ms, 4), kernels_gbs=round(nbytes / k_ms / 1e6, 1),
                   kernels_iters=k_iters, prepare_ms=round(p_ms, 4), prepare_host_ms=round(p_host_ms, 4), prepare_iters=p_iters,
                   numpy_ms_per_sample=round(ref_ms, 2), numpy_samples=n_ref, device=torch.cuda.get_device_name(0))
        print(json.dumps(res), flush=True)
        results.append(res)
        del store, batcher, out, ch, table
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
