"""Times image-view preparation on the device (bridgeqa_amd.view_data over csrc/view_prep.hip) at the sizes the project uses,
the PatchEmbed unfold and cast it makes unnecessary, and the host definition (Pillow resize, torch normalise) on one core of
the same machine.

    python tools/bench_view_prep.py [--out profiles/view_prep.json] [--seconds 1.5]

Per case it prints one JSON line:
  prepare_ms      device ms per batch of ViewBatcher.prepare(index on the device, out=...): ONE launch, nothing else enqueued;
                  device events around `iters` back-to-back batches after a warm-up, iters chosen so the window exceeds --seconds
  gbs             algorithmic bytes / prepare_ms.  Algorithmic bytes: the frames' bytes read once (3 H W per view) and the
                  output written once
  bit_equal       view 0 of the batch against tests/viewprep_ref.py at this very size
  unfold_cast_ms  (fp32 NCHW cases at 480) what vit.PatchEmbed.forward and ops.linear run on that batch before the GEMM when
                  they are handed fp32 NCHW images: the reshape / permute / reshape copy into patch rows, then .to(bfloat16)
  pillow_ms_per_view  Image.resize(BICUBIC) + ToTensor / Normalize with torch on one core (threads set to 1), frame in memory;
                  null where Pillow is not installed
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

# (name, views in the batch, H, W, size, dtype, layout)
CASES = (("16 x 240x320 -> 480, fp32 NCHW", 16, 240, 320, 480, "float32", "nchw"),
         ("16 x 240x320 -> 480, bf16 patches", 16, 240, 320, 480, "bfloat16", "patches"),
         ("16 x 968x1296 -> 480, fp32 NCHW", 16, 968, 1296, 480, "float32", "nchw"),
         ("16 x 968x1296 -> 480, bf16 patches", 16, 968, 1296, 480, "bfloat16", "patches"),
         ("256 x 240x320 -> 384, fp32 NCHW", 256, 240, 320, 384, "float32", "nchw"),
         ("256 x 968x1296 -> 384, fp32 NCHW", 256, 968, 1296, 384, "float32", "nchw"))


def timed(fn, seconds):
    """-> (device ms per call, calls): warm-up, a probe of 5 calls, then a window longer than `seconds`"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    iters = max(20, int(seconds / max((time.perf_counter() - t0) / 5, 1e-6)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, iters


def frames_of(H, W, n):
    """n distinct frames with an image's statistics: a smooth field plus noise"""
    rs = np.random.RandomState(H + W)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = 128 + 90 * np.sin(x / (17.0 + i)) * np.cos(y / (23.0 + i))
        out.append(np.clip(base[:, :, None] + rs.randint(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def pillow_ms(frame, size, repeats):
    try:
        from PIL import Image
    except ImportError:
        return None
    from bridgeqa_amd.view_data import CLIP_MEAN, CLIP_STD
    m, s = torch.tensor(CLIP_MEAN)[:, None, None], torch.tensor(CLIP_STD)[:, None, None]
    img = Image.fromarray(frame)
    t0 = time.perf_counter()
    for _ in range(repeats):
        r = torch.from_numpy(np.asarray(img.resize((size, size), Image.BICUBIC)).copy())
        r.permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(m).div_(s)
    return (time.perf_counter() - t0) * 1e3 / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames in the store (the batch cycles through them)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_view_prep: needs a GPU (there is no CPU fallback and no CPU timing of the kernel)")
    import viewprep_ref as R
    from bridgeqa_amd import _ext
    from bridgeqa_amd.view_data import ViewBatcher, ViewStore
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    results, stores = [], {}
    for name, n, H, W, size, dtype, layout in CASES:
        if (H, W) not in stores:
            stores.clear()
            torch.cuda.empty_cache()
            stores[(H, W)] = (frames_of(H, W, args.distinct),)
            stores[(H, W)] += (ViewStore(stores[(H, W)][0], dev),)
        frames, store = stores[(H, W)]
        dt = getattr(torch, dtype)
        b = ViewBatcher(store, size, dtype=dt, layout=layout)
        index = torch.arange(n, device=dev) % len(store)
        out = b.empty(n)
        before = _ext.VIEW_CALLS[0]
        ms, iters = timed(lambda: b.prepare(index, out=out), args.seconds)
        launches = (_ext.VIEW_CALLS[0] - before) / (iters + 8)
        want = R.preprocess(frames[0], size, size).to(dt)
        want = R.to_patches(want, 16) if layout == "patches" else want
        equal = bool(torch.equal(out["images"][0, 0].cpu().view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                                 want.view(torch.int16 if dt == torch.bfloat16 else torch.int32)))
        nbytes = n * 3 * H * W + out["images"].numel() * out["images"].element_size()
        res = dict(case=name, views=n, H=H, W=W, size=size, dtype=dtype, layout=layout, tile_rows=b.tile_rows,
                   lds_bytes=4096 + b.lds_rows * 3 * size, launches_per_batch=launches, algorithmic_mb=round(nbytes / 1e6, 2),
                   output_mb=round(out["images"].numel() * out["images"].element_size() / 1e6, 2), prepare_ms=round(ms, 4),
                   gbs=round(nbytes / ms / 1e6, 1), iters=iters, bit_equal=equal, device=torch.cuda.get_device_name(0))
        if layout == "nchw" and size == 480:
            x = out["images"][:, 0]

            def unfold_cast():
                B, C = x.shape[:2]
                p = x.reshape(B, C, size // 16, 16, size // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, -1, C * 256)
                return p.to(torch.bfloat16)
            res["unfold_cast_ms"], res["unfold_cast_iters"] = (round(v, 4) for v in timed(unfold_cast, args.seconds))
        if layout == "nchw":
            host = pillow_ms(frames[0], size, 8)
            res["pillow_ms_per_view"] = host and round(host, 2)
        print(json.dumps(res), flush=True)
        results.append(res)
        del b, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
