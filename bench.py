#!/usr/bin/env python
"""bench.py -- BASELINE.json's metric on synthetic data.

    python bench.py [--gpus N --steps K --warmup W] [--workload c2|c3] [--cin 132] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one training pass (forward + backward + AdamW step) of the hot path over one synthetic
batch that is already resident in HBM: B=16 scenes x 40000 points (xyz + C_in features), and for
workload c3 additionally one 512x512 view + question/answer ids per scene.  One process per GPU;
each rank owns its own B=16 batch (weak scaling), gradients are all-reduced over RCCL.
Rank 0 prints ONE JSON line: the headline (`value` in samples/s, `ms_per_step`) and the configuration it was measured on.
That is all a plain run does after its timed steps.  `--full` adds, after the timed steps, what takes runs of its own:
`roofline` for the dominant kernel and the per-kernel sub-rooflines (dedicated launches), `loop_reference` (the
reference's unchanged loop, timed again) and `cpu_baseline` (the CPU oracle port timed on a bounded sample; N=1 only).
`--dump-outputs DIR` also writes what the last timed step computed as DIR/<name>.npy; that step starts from the seeded
initial weights and a fresh optimizer (restored off the clock), so its inputs are the same in every run and two builds run
with the same arguments can be compared array by array.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {
    "c2": "c2: DET-stage hot path (VoteNet backbone + voting + vote-cluster/proposal), fwd+bwd+AdamW, "
          "the reference's detection loss (vote/objectness/box/sem-cls) on synthetic boxes",
    "c3": "c3: VQA-stage hot path (c2 + ViT-B/16 on one 512x512 view + paralleltwin MED fusion + shared LM "
          "answer decoder on both streams), fwd+bwd+AdamW, LM answer loss + the reference's detection loss "
          "(vote/objectness/box/sem-cls) on synthetic boxes",
}
WORKLOADS["c5"] = ("c5 (one rank's share): " + WORKLOADS["c3"][4:] + " -- at B=32 x 80000 points + one 1024x1024 view "
                   "(4097 image tokens) per scene")
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
DUMP_SAMPLE = 1 << 22          # --dump-outputs: elements kept per array (16 MB in float32)
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: all arrays together


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=os.environ.get("BQ_WORKLOAD", "auto"), choices=["auto", "c2", "c3", "c5"],
                    help="auto = c3 (the configuration BASELINE.json's metric is quoted on); c5 = one rank's share of the "
                         "large-context configuration (B=32 x 80000 points + 1024^2 views, 4097 image tokens)")
    ap.add_argument("--cin", type=int, default=132, help="per-point feature channels (README recipe: 128+3+1)")
    ap.add_argument("--batch", type=int, default=None, help="scenes per rank (default 16; c5: 32)")
    ap.add_argument("--points", type=int, default=None, help="points per scene (default 40000; c5: 80000)")
    ap.add_argument("--image", type=int, default=None, help="view side in pixels (default 512; c5: 1024)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: roofline and per-kernel "
                         "figures from launches of their own, the reference's loop (loop_reference) and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: leave out the CPU baseline")
    ap.add_argument("--no-geometry-prefetch", action="store_true",
                    help="c2: compute the sampling / grouping indices inside the step instead of one step ahead on a second stream")
    ap.add_argument("--dp-path", action="store_true", help="use the data-parallel step structure even on one GPU")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="process-group backend (nccl = RCCL; gloo only for --share-device validation runs)")
    ap.add_argument("--grad-exchange", choices=["all_reduce", "reduce_scatter"], default="all_reduce",
                    help="data parallel: one all-reduce per gradient group (RCCL picks the algorithm), or reduce-scatter + "
                         "all-gather written out (SURVEY §8e)")
    ap.add_argument("--share-device", action="store_true",
                    help="VALIDATION ONLY: every rank uses cuda:0 (with --backend gloo: RCCL refuses two ranks on one GPU) -- "
                         "runs the N > 1 control flow (per-rank batches, per-phase gradient groups, buffer broadcast, replica "
                         "check) on a 1-GPU box; the throughput of such a run means nothing")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the whole train step (forward + backward + fused AdamW) from one HIP graph; "
                         "auto = on for a single GPU")
    ap.add_argument("--no-text-prologue", dest="text_prologue", action="store_false",
                    help="A/B: the question / answer embeddings inside the fusion phase (as before round 4) instead of as phases "
                         "of their own beside the image encoder / the image backward")
    ap.add_argument("--loop", choices=["phased", "reference"], default="phased",
                    help="c3: phased = pipeline.PhasedTrainStep (the measured step structure, the headline); reference = the "
                         "reference's own loop, unchanged -- data_dict = model(data_dict); loss = get_loss(...); "
                         "optimizer.zero_grad(); loss.backward(); optimizer.step() (lib/solver.py:463-595) -- with HIP-graph "
                         "replay behind model() and loss.backward() (bridgeqa_amd/graphed.py; --graph off: kernel by kernel)")
    ap.add_argument("--no-wrap-loss", dest="wrap_loss", action="store_false",
                    help="--loop reference: leave the loss function eager (default: graphed.wrap_loss around it)")
    ap.add_argument("--no-prefetch", dest="no_prefetch", action="store_true",
                    help="reference loop: no graphed.prefetch_loader (every step computes its own sampling / grouping indices)")
    ap.add_argument("--eager-optimizer", dest="eager_optimizer", action="store_true",
                    help="reference loop: optimizer.step() launched eagerly (default: graphed.wrap_optimizer)")
    ap.add_argument("--no-loop-reference", dest="no_loop_reference", action="store_true",
                    help="--full c3 run: skip the second measurement (the reference's unchanged loop under graphed, "
                         "reported as `loop_reference` on the same JSON line)")
    ap.add_argument("--cpu-scenes", type=int, default=2, help="--full: scenes in the bounded CPU-baseline sample")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="--full: threads of the CPU baseline (0: min(os.cpu_count(), 32))")
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16",
                    help="arithmetic of the dense layers: bf16 = the HIP kernel path (MFMA GEMMs, point-major detector); "
                         "f32 = the reference composition on torch ops (c2 only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (its loss, the parameters the "
                         "optimizer left, their gradients, the floating-point buffers) as DIR/<name>.npy, %d MB at most"
                         % (DUMP_MAX_BYTES >> 20))
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    big = args.workload == "c5"
    args.batch = args.batch or (32 if big else 16)
    args.points = args.points or (80000 if big else 40000)
    args.image = args.image or (1024 if big else 512)
    return args


def synth_batch(B, N, cin, seed, device):
    """SURVEY.md §8d synthetic inputs: xyz ~ U([0,8]x[0,8]x[0,3]) m, features ~ N(0,1), seed 42."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g) * torch.tensor([8.0, 8.0, 3.0])
    feats = torch.randn(B, N, cin, generator=g)
    return torch.cat([xyz, feats], -1).contiguous().to(device)


def build_model(workload, cin, image):
    from bridgeqa_amd.hotpath import ScanQAHotPath
    if workload == "c2":
        return ScanQAHotPath(input_feature_dim=cin, use_blip=False)
    return ScanQAHotPath(input_feature_dim=cin, use_blip=True, blip_kwargs=dict(image_size=image))


def synth_text(B, L, La, seed, device):
    """question ids (B,L) ~ U{1000..30521}, [ENC] at 0 (set by the model), 0-6 trailing pads;
    answers (B,La)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(1000, 30522, (B, L), generator=g)
    qm = torch.ones(B, L, dtype=torch.long)
    for b in range(B):
        pad = int(torch.randint(0, 7, (1,), generator=g))
        if pad:
            q[b, L - pad:] = 0
            qm[b, L - pad:] = 0
    a = torch.randint(1000, 30522, (B, La), generator=g)
    am = torch.ones(B, La, dtype=torch.long)
    return ({"input_ids": q.to(device), "attention_mask": qm.to(device)},
            {"input_ids": a.to(device), "attention_mask": am.to(device)})


DET_LOSS_WEIGHTS = dict(vote_loss=1.0, objectness_loss=0.5, box_loss=1.0, sem_cls_loss=0.1)  # scripts/train.py:97-103
NUM_GT_BOXES, MAX_NUM_OBJ = 8, 128  # SURVEY §8d synthetic labels; lib/dataset.py:31


def det_config():
    """the members of the reference's ScannetDatasetConfig that the losses read, at ScanQAHotPath's defaults"""
    import types
    import numpy as np
    return types.SimpleNamespace(num_heading_bin=1, num_size_cluster=18, num_class=18, mean_size_arr=np.ones((18, 3)))


def synth_labels(xyz, seed):
    """8 random axis-aligned boxes per scene with the label fields of lib/dataset.py:553-577 (centre,
    heading class / residual = 0, size class / residual w.r.t. mean_size_arr = 1, semantic class, box mask, padded to
    MAX_NUM_OBJ at -100 like dataset.py:423) and per-point votes towards the centre of the box a point lies in."""
    B, N, _ = xyz.shape
    g = torch.Generator().manual_seed(seed)
    centre = torch.full((B, MAX_NUM_OBJ, 3), -100.0)
    size = torch.ones(B, MAX_NUM_OBJ, 3)
    centre[:, :NUM_GT_BOXES] = torch.rand(B, NUM_GT_BOXES, 3, generator=g) * torch.tensor([8.0, 8.0, 3.0])
    size[:, :NUM_GT_BOXES] = torch.rand(B, NUM_GT_BOXES, 3, generator=g) * 1.2 + 0.3
    cls = torch.zeros(B, MAX_NUM_OBJ, dtype=torch.long)
    cls[:, :NUM_GT_BOXES] = torch.randint(0, 18, (B, NUM_GT_BOXES), generator=g)
    mask = torch.zeros(B, MAX_NUM_OBJ)
    mask[:, :NUM_GT_BOXES] = 1
    c, h = centre[:, None, :NUM_GT_BOXES], size[:, None, :NUM_GT_BOXES] / 2
    inside = ((xyz[:, :, None] - c).abs() <= h).all(-1)                     # (B, N, 8)
    first = inside.float().argmax(-1)                                       # first box containing the point
    vote = torch.gather(centre[:, :NUM_GT_BOXES], 1, first[..., None].expand(-1, -1, 3)) - xyz
    vmask = inside.any(-1)
    vote = torch.where(vmask[..., None], vote, torch.zeros_like(vote))
    return {"center_label": centre, "heading_class_label": torch.zeros(B, MAX_NUM_OBJ, dtype=torch.long),
            "heading_residual_label": torch.zeros(B, MAX_NUM_OBJ), "size_class_label": cls,
            "size_residual_label": size - 1.0, "sem_cls_label": cls.clone(), "box_label_mask": mask,
            "vote_label": vote.repeat(1, 1, 3), "vote_label_mask": vmask.long()}


def det_loss(dd):
    """the reference's detection loss (lib/loss_helper.py get_loss, detection terms: vote + objectness + box + sem-cls,
    scripts/train.py weights, x10) through bridgeqa_amd/loss_helper.py"""
    from bridgeqa_amd.loss_helper import get_detection_loss
    return get_detection_loss(dd, det_config(), DET_LOSS_WEIGHTS)[0]


def path_roofline(args, workload):
    """SURVEY.md §8d path-level bound: t_min = sum over ops of max(bytes / HBM peak, flops / MFMA peak), from the
    ALGORITHMIC work of one B-sample train step (train = 3 x forward flops; FPS / ball query in their
    streaming-equivalent bytes, grouped tensors in true bytes).  Returns (t_min_ms, detail)."""
    B, N = args.batch, args.points
    stages = ((N, 2048, 64), (2048, 1024, 32), (1024, 512, 16), (512, 256, 16), (1024, 256, 16))
    chans = (args.cin, 128, 256, 256, 256)
    fps_b = sum(20.0 * n * (m - 1) * B for n, m, _ in stages)
    bq_b = sum(12.0 * n * m * B for n, m, _ in stages)
    grp_b = sum(4.0 * (c + 3) * m * s_ * B for (n, m, s_), c in zip(stages, chans))
    det_flops = 3.0 * 13.4e9 * B * (1.0 if args.cin > 1 else 11.2 / 13.4)
    flops = det_flops
    if workload == "c3":
        P = (args.image // 16) ** 2 + 1
        vit = 12 * (2 * P * 768 * 2304 + 4 * P * P * 768 + 2 * P * 768 * 768 + 4 * P * 768 * 3072) + 2 * (P - 1) * 768 * 768
        twin, dec = 46.3e9, 2 * 1.8e9   # L = 20, La = 5
        flops += 3.0 * (vit + twin + dec) * B
    t_bytes = (fps_b + bq_b + grp_b) / (HBM_PEAK_GBS * 1e9)
    t_flops = flops / 2.5e15
    return (t_bytes + t_flops) * 1e3, {"hbm_bytes": fps_b + bq_b + grp_b, "mfma_flops": flops,
                                       "hbm_peak_GBs": HBM_PEAK_GBS, "mfma_peak_TFLOPs": 2500.0}


def fusion_loss(dd):
    # LM answer loss of both streams (blip_vqa_3d.py:305-343); the fused 2D/3D states feed the reference's downstream
    # heads (qa_module.py:735-754): keep their backward (lowrank projections + bilinear fuse) in the timed step
    return dd["blip_loss"] + dd["fused_feat"].float().square().mean() * 1e-3


def total_loss(dd):
    loss = det_loss(dd)
    if "blip_loss" in dd:
        loss = loss + fusion_loss(dd)
    return loss


class OpTimer(object):
    """HIP-event timing of the native operators on the stream they are launched on."""

    def __init__(self):
        self.records = []

    def wrap(self, ext, names):
        self._orig = {n: getattr(ext, n) for n in names}
        for n in names:
            def timed(*a, _n=n, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = self._orig[_n](*a, **k)
                e.record()
                self.records.append((_n, tuple(a[0].shape), s, e))
                return out
            setattr(ext, n, timed)
        self._ext = ext

    def unwrap(self):
        for n, f in self._orig.items():
            setattr(self._ext, n, f)

    def summary(self):
        """{(op, shape): (median ms, count)} -- the median: in an eager re-run the stream can run dry between the two events
        of a launch (the host allocating, a first-use initialisation), and one such pair moved a 16 us launch's MEAN to
        10 ms on the c2 line of round 3"""
        agg = {}
        for n, shape, s, e in self.records:
            agg.setdefault((n, shape), []).append(s.elapsed_time(e))
        return {k: (sorted(v)[len(v) // 2], len(v)) for k, v in agg.items()}


def _flat_sample(tensors, seed):
    """`tensors` (None = a zero tensor of `numel` elements) flattened and concatenated in order, as float32 on the host: every
    element when there are at most DUMP_SAMPLE, else DUMP_SAMPLE of them at sorted positions drawn from a generator seeded
    with `seed` -- the same positions in every run with the same arguments.  Items are (tensor or None, numel)."""
    import numpy as np
    total = sum(n for _, n in tensors)
    pos = None
    if total > DUMP_SAMPLE:
        g = torch.Generator().manual_seed(seed)
        pos = torch.randint(0, total, (DUMP_SAMPLE,), generator=g).sort().values
    out, off = [], 0
    for t, n in tensors:
        if pos is None:
            lo, hi, take = 0, n, None
        else:
            lo, hi = torch.searchsorted(pos, torch.tensor([off, off + n])).tolist()
            take = pos[lo:hi] - off
        if hi > lo:
            if t is None:
                out.append(torch.zeros(hi - lo))
            else:
                flat = t.detach().reshape(-1)
                out.append((flat if take is None else flat[take.to(flat.device)]).float().cpu())
        off += n
    return torch.cat(out).numpy() if out else np.zeros(0, np.float32)


def initial_state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def restore_initial_state(model, opt, state):
    """--dump-outputs, before the last timed step (off the clock): parameters and buffers back to the seeded values the run
    started from and the optimizer back to fresh (zero moments and step count), in place, so that the captured graphs keep
    their operands.  The steps before it sum some gradients with fp32 atomics, and this loss turns rounding-level
    differences into different trajectories; from the same state the step itself reproduces to rounding.  With this the
    dumped step has the same inputs in every run.  (As PhasedTrainStep.capture puts back the state of its warm-up steps.)"""
    from bridgeqa_amd import fusion_ops
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(state[k])
        for st in opt.state.values():
            for t in st.values():
                if torch.is_tensor(t):
                    t.zero_()
    fusion_ops.refresh_shadows(only_with_grad=False)   # the bf16 operand copies of the restored weights
    fusion_ops.mark_transposed_stale()
    torch.cuda.synchronize()


def dump_outputs(path, model, loss):
    """--dump-outputs: what the last timed step handed its caller -- the loss, the parameters the optimizer left, their
    gradients (zero where a parameter received none) and the floating-point buffers (BatchNorm running statistics) -- as
    path/<name>.npy.  Called right after the timed steps, before anything else runs on the model."""
    import numpy as np
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()
    params = [p for _, p in model.named_parameters()]
    arrays = {
        "loss": np.asarray([loss.detach().double().item()], np.float64),
        "parameters": _flat_sample([(p, p.numel()) for p in params], 1),
        "gradients": _flat_sample([(p.grad, p.numel()) for p in params], 1),   # (same seed: the same positions)
        "buffers": _flat_sample([(b, b.numel()) for _, b in model.named_buffers() if b.is_floating_point()], 2),
    }
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_MAX_BYTES
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def make_batch(args, workload, B, seed, device):
    batch = {"point_clouds": synth_batch(B, args.points, args.cin, seed, device), "phase": "train"}
    batch.update({k: v.to(device) for k, v in synth_labels(batch["point_clouds"][..., :3].cpu(), seed + 7).items()})
    if workload == "c3":
        g = torch.Generator().manual_seed(seed + 1)
        batch["images"] = torch.randn(B, 1, 3, args.image, args.image, generator=g).to(device)
        batch["question"], batch["answer"] = synth_text(B, 20, 5, seed + 2, device)
    return batch


def cpu_baseline(args, workload):
    """The hot path on the host cores: bridgeqa_amd's Python layers over the CPU oracle backend
    (oracle/ -- allowed here as the reported baseline only) + torch-CPU fp32 for the dense layers."""
    from bridgeqa_amd import pointnet2_utils
    cores = int(getattr(args, "cpu_threads", 0) or 0) or min(os.cpu_count() or 1, 32)  # (default: beyond ~32 threads this
    #                                                   workload only adds contention; --cpu-threads N runs any other count)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    from oracle import pn2_oracle
    torch.set_num_threads(cores)
    prev = pointnet2_utils.set_backend(pn2_oracle)
    try:
        from bridgeqa_amd import fusion_ops
        prev_dt = fusion_ops.set_compute_dtype(torch.float32)
        torch.manual_seed(0)
        model = build_model(workload, args.cin, args.image)
        opt = torch.optim.AdamW(model.parameters(), lr=5e-4)
        B = args.cpu_scenes
        batch = make_batch(args, workload, B, 42, "cpu")
        times = []
        for it in range(4):  # one warm-up + 3 timed steps
            t0 = time.time()
            opt.zero_grad(set_to_none=True)
            loss = total_loss(model(dict(batch)))
            loss.backward()
            torch.nn.utils.clip_grad_value_(model.parameters(), 1.0)
            opt.step()
            times.append(time.time() - t0)
        dt = sum(times[1:]) / len(times[1:])
        fusion_ops.set_compute_dtype(prev_dt)
    finally:
        pointnet2_utils.set_backend(prev)
    model_name, phys = cpu_info()
    return {"value": round(B / dt, 4), "unit": "samples/s", "cores": cores, "kind": "port",
            "cpu_model": model_name, "physical_cores": phys, "logical_cpus": os.cpu_count(), "threads_used": cores,
            "sample": "%s hot path fwd+bwd+clip+AdamW, %d scenes x %d pts, C_in=%d, fp32, mean of 3 timed steps after "
                      "1 warm-up (oracle ops with OpenMP + torch-CPU dense layers on %d threads)"
                      % (workload, B, args.points, args.cin, cores),
            "deviation_from_BASELINE_md_2": "BASELINE.md section 2 plans os.cpu_count() threads at B = 16.  Bounded here on purpose: "
                                            "4 steps at B = 16 take ~150 s of host time on this path (the contract asks for a "
                                            "10-30 s sample inside the default run), and samples/s does not depend on B on the "
                                            "CPU (every operator and dense layer is per-sample work; --cpu-scenes 16 runs the "
                                            "planned size); threads are capped at 32 because the oracle's OpenMP loops and "
                                            "torch-CPU's GEMMs at these sizes get SLOWER beyond ~32 threads on the 128-core host "
                                            "(memory-bound, cross-CCD traffic): 32 is the fastest setting measured, i.e. the "
                                            "baseline is not handicapped"}


def cpu_info():
    """(model name, physical core count) of the host the baseline ran on, from /proc/cpuinfo"""
    name, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                name = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None:
                cores.add((phys, core))
        if phys is not None:
            cores.add((phys, core))
    except OSError:
        pass
    return name, len(cores) or None


VIT_GEMMS = (("qkv", 2304, 768), ("proj", 768, 768), ("fc1", 3072, 768), ("fc2", 768, 3072))
PROFILE_PMC = os.path.join(ROOT, "profiles", "r06_gemm_pmc.jsonl")       # tools/run_gemm_pmc.sh -> tools/pmc_summary.py --json
PROFILE_STATS = os.path.join(ROOT, "profiles", "r06_c3_kernel_stats.csv")  # rocprofv3 --kernel-trace --stats of this bench
PROFILE_ROWS = 16400   # the committed counter / in-step records were taken at c3's token count (B = 16 x 1025): they are
#                        attached to a bench line only when the run has the same M (the c5 line divided c3's bytes)
# kernel instantiation each launch form runs as (for the in-step averages of the committed profile)
GEMM_KERNELS = {"fwd": "gemm128_kernel<false, false, 1, false, 16>", "fwd_gelu": "gemm128_kernel<false, false, 2, false, 16>",
                "dx": "gemm128_kernel<false, false, 0, false, 16>", "dx_dgelu": "gemm128_kernel<false, false, 3, false, 16>",
                "dw": "gemm256_kernel<true, true, 0, true>"}


def _event_median_ms(fn, reps=10, warm=3):
    """median over `reps` single launches, HIP events on the stream the launch goes to (the current one)"""
    for _ in range(warm):
        fn()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b_) for a, b_ in evs)[len(evs) // 2]


def _profile_records():
    """(per-launch PMC records by label, in-step kernel averages by name) from the committed profiles, {} when absent"""
    pmc, stats = {}, {}
    try:
        for line in open(PROFILE_PMC):
            r = json.loads(line)
            pmc.setdefault(r["label"], []).append(r)
    except OSError:
        pass
    try:
        import csv
        for r in csv.DictReader(open(PROFILE_STATS)):
            stats[r["Name"]] = (float(r["AverageNs"]) / 1e3, int(r["Calls"]))
    except OSError:
        pass
    return pmc, stats


def gemm_roofline(args, dev):
    """The dominant dense kernels of the step: the launches ONE ViT block runs forward (qkv / proj / fc1 + GELU / fc2, with
    the epilogues and the tile the step uses) and backward (their input gradients, fc2's with the GELU derivative), at this
    run's token count -- HIP events around each launch on the stream it is launched on (the step itself replays them from
    HIP graphs, where no event can be placed: these are the SAME kernels on the SAME shapes, launched right after the timed
    region) -- and the grouped weight-gradient launch of all 12 blocks.  flops = 2 M N K per launch."""
    from bridgeqa_amd import _ext
    M = args.batch * ((args.image // 16) ** 2 + 1)
    g = torch.Generator().manual_seed(5)
    rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dev).to(torch.bfloat16)
    pmc, stats = _profile_records() if M == PROFILE_ROWS else ({}, {})
    out, tot_f, tot_t, tot_alg, tot_fetch, tot_write, tot_prof = [], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    prof_missing = []

    def add(label, form, fn, fl, alg_bytes, N, K):
        nonlocal tot_f, tot_t, tot_alg, tot_fetch, tot_write, tot_prof
        ms = _event_median_ms(fn)
        rec = {"launch": label, "M": M, "N": N, "K": K, "us": round(ms * 1e3, 1), "TFLOPs": round(fl / ms / 1e9, 1),
               "frac": round(fl / ms / 1e9 / 2500.0, 4), "algorithmic_bytes": alg_bytes}
        kn = "void bq::%s(bq::GemmArgs)" % GEMM_KERNELS[form]
        if kn in stats:
            rec["in_step_avg_us_all_shapes_of_this_kernel"] = round(stats[kn][0], 1)
        p = [r for r in pmc.get(label, []) if r.get("fetch_bytes") is not None]
        if p:
            tsum = sum(r["avg_us"] for r in p)
            rec["pmc"] = {"us": tsum,   # (several kernels per label: the weight-gradient flush; utilisation time-weighted)
                          "mfma_util": round(sum((r.get("mfma_util") or 0.0) * r["avg_us"] for r in p) / tsum, 4),
                          "hbm_read_bytes": sum(r["fetch_bytes"] for r in p), "hbm_write_bytes": sum(r["write_bytes"] for r in p)}
            tot_fetch += rec["pmc"]["hbm_read_bytes"]
            tot_write += rec["pmc"]["hbm_write_bytes"]
            tot_prof += tsum
        else:
            prof_missing.append(label)
        out.append(rec)
        tot_f += fl; tot_t += ms; tot_alg += alg_bytes

    for name, N, K in VIT_GEMMS:
        x, w, dy, pre = rnd(M, K), rnd(N, K, sc=0.05), rnd(M, N), rnd(M, K)
        wt = w.t().contiguous()   # the step's input-gradient launches read the K-contiguous copy (fusion_state.transposed_shadow)
        b = torch.randn(N, generator=g).to(dev)
        fl = 2.0 * M * N * K
        if name == "fc1":
            # (algorithmic bytes count ONE output: the activation is what the layer computes; the launch also stores the
            # pre-activation for the backward -- the counter bytes show it)
            add("fwd_fc1_gelu", "fwd_gelu", lambda: _ext.gemm_fwd(x, w, b, gelu=True), fl, 2.0 * (M * K + N * K + M * N), N, K)
            out[-1]["note"] = "writes two (M, N) outputs (pre-activation for the backward + activation); algorithmic bytes count one"
        else:
            add("fwd_" + name, "fwd", lambda: _ext.gemm_fwd(x, w, b), fl, 2.0 * (M * K + N * K + M * N), N, K)
        if name == "fc2":
            add("dx_fc2_dgelu", "dx_dgelu", lambda: _ext.gemm_dx(dy, w, pre_act=pre, wt=wt), fl, 2.0 * (M * N + N * K + 2 * M * K), N, K)
        else:
            add("dx_" + name, "dx", lambda: _ext.gemm_dx(dy, w, wt=wt), fl, 2.0 * (M * N + N * K + M * K), N, K)
        del x, w, dy, pre, wt
    # the weight gradients exactly as the step issues them: the deferred flush of the image backward (fusion_wgrad: launch
    # plan over the 256-tile problems, bias gradients from the same launches, the planner's small problems on the 64-tile kernel)
    from bridgeqa_amd import fusion_wgrad
    items, params, fl, by = [], [], 0.0, 0.0
    for blk in range(12):
        for name, N, K in VIT_GEMMS:
            wp, bp = torch.nn.Parameter(torch.empty(N, K, device=dev)), torch.nn.Parameter(torch.empty(N, device=dev))
            params += [wp, bp]
            items.append((rnd(M, N), rnd(M, K), [wp], [bp]))
            fl += 2.0 * M * N * K
            by += 2.0 * M * (N + K) + 4.0 * N * K

    def flush():
        for p_ in params:
            p_.grad = None
        fusion_wgrad.flush_deferred_items(items)
    add("dw_grouped48", "dw", flush, fl, by, 0, 0)
    out[-1]["note"] = ("all 48 weight gradients (+ bias gradients) of the 12 blocks through fusion_wgrad.flush_deferred_items: "
                       "the launch plan the step uses (two 256-tile launches + the planner's small problems on the 64-tile kernel)")
    traffic = ({"hbm_read_bytes": tot_fetch, "hbm_write_bytes": tot_write, "algorithmic_bytes": tot_alg,
                "ratio": round((tot_fetch + tot_write) / tot_alg, 3), "file": "profiles/r06_gemm_pmc.jsonl",
                "method": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, one launch form per process; read = 2 x "
                          "FETCH_SIZE x 1024 (gfx950 tallies a 128-B request as 64 B), write = WRITE_SIZE x 1024 "
                          "(MI355X_MICROARCH.md, HBM); fabric-side counters: Infinity-Cache hits are included"}
               if (tot_fetch and not prof_missing) else None)
    # the same fraction from the DURATIONS of the committed trace pass (rocprofv3 kernel trace, one launch form per
    # process) next to the live HIP-event medians `frac` uses: a reader can recompute either from its own source
    prof = ({"us_total": round(tot_prof, 1), "frac": round(tot_f / (tot_prof * 1e-6) / 1e12 / 2500.0, 4),
             "file": "profiles/r06_gemm_pmc.jsonl (avg_us of the trace pass)"} if (tot_prof and not prof_missing) else None)
    return out, tot_f, tot_t, traffic, prof


def _attn_pmc(threads, path="profiles/r06_attn_pmc.txt"):
    """MFMA-busy fractions of the three attention kernels at THIS run's shape, read back from the committed counter summary
    (tools/run_attn_pmc.sh -> tools/pmc_summary.py: per kernel and launch shape a '<name>  grid <threads>' line followed by
    the counters and a '=> MFMA utilisation X %' line); `threads` = B * H * ceil(L / 128) workgroups * 256"""
    full = os.path.join(os.path.dirname(os.path.abspath(__file__)), path)
    if not os.path.exists(full):
        return None
    out, cur = {"file": path, "grid_threads": threads}, None
    for line in open(full):
        for key, pat in (("fwd", "attn_fwd_kernel"), ("dq", "attn_bwd_dq_kernel"), ("dkv", "attn_bwd_dkv_kernel")):
            if pat in line:
                cur = key if line.rstrip().endswith("grid %d" % threads) else None
        if "MFMA utilisation" in line and cur is not None and cur + "_mfma_busy" not in out:
            try:
                out[cur + "_mfma_busy"] = float(line.split("MFMA utilisation")[1].split("%")[0]) / 100.0
            except ValueError:
                pass
            cur = None
    return out


def attn_roofline(args, dev):
    """The fused attention kernels (csrc/attn.hip) at the ViT shape of this run: forward and backward of one block,
    flops = 4 B H L^2 64 forward, 2.5 x that backward (the minimal count; the kernels recompute S: 3.5 x executed)"""
    from bridgeqa_amd import _ext
    B, H, L = args.batch, 12, (args.image // 16) ** 2 + 1
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(B, L, 3, H, 64, generator=g).to(dev).to(torch.bfloat16)
    go = torch.randn(B, L, H, 64, generator=g).to(dev).to(torch.bfloat16)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    tf = _event_median_ms(lambda: _ext.attn_fwd(q, k, v, 0.125))
    o, lse = _ext.attn_fwd(q, k, v, 0.125)
    dqkv = torch.empty_like(qkv)
    tb = _event_median_ms(lambda: _ext.attn_bwd(q, k, v, o, lse, go, 0.125, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]))
    fl = 4.0 * B * H * L * L * 64
    return {"kernel": "bq::attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel (csrc/attn.hip), ViT block, B=%d H=12 "
                      "L=%d D=64" % (B, L), "bound": "mfma", "peak": 2500.0, "unit": "TFLOP/s",
            "fwd": {"us": round(tf * 1e3, 1), "achieved": round(fl / tf / 1e9, 1), "frac": round(fl / tf / 1e9 / 2500.0, 4)},
            "bwd": {"us": round(tb * 1e3, 1), "achieved": round(2.5 * fl / tb / 1e9, 1),
                    "frac": round(2.5 * fl / tb / 1e9 / 2500.0, 4), "executed_flops_factor": 3.5},
            "achieved": round(3.5 * fl / (tf + tb) / 1e9, 1), "frac": round(3.5 * fl / (tf + tb) / 1e9 / 2500.0, 4),
            "pmc": _attn_pmc(B * H * -(-L // 128) * 256),
            "timed_on": "dedicated launches after the timed region, HIP events on the launch stream, median of 10"}


class _StaticLoader(object):
    """the benchmark's stand-in for the reference's DataLoader: the same synthetic batch `n` times (what the headline
    replays too); a fresh dict per iteration, as a loader's collate function returns"""

    def __init__(self, batch, n):
        self.batch, self.n = batch, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for _ in range(self.n):
            yield dict(self.batch)


def run_reference_loop(args, model, batch, dev, use_graph, steps, warmup, trace=False, dump_dir=None):
    """The reference's training iteration as its solver writes it (lib/solver.py:463-595 _feed / _forward / _backward,
    scripts/train.py:410-417), the loop BODY unchanged: forward through the module API, the loss outside the model,
    zero_grad / backward / (clip inside) optimizer.step.  With graphs: graphed.enable(model, optimizer) replays HIP graphs
    behind model(), loss.backward() and optimizer.step(); graphed.wrap_loss around the loss function;
    graphed.prefetch_loader around the loader (the next batch's sampling / grouping indices under this step's fusion).
    -> dict for the JSON line"""
    from bridgeqa_amd import graphed
    from bridgeqa_amd.optim import FusedAdamW
    state0 = initial_state(model) if dump_dir else None
    opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=1e-5, grad_clip_value=1.0)
    loss_fn = total_loss
    prefetch = use_graph and not getattr(args, "no_prefetch", False)
    if use_graph:
        graphed.enable(model, optimizer=None if getattr(args, "eager_optimizer", False) else opt)
        # (the solver's `from lib.loss_helper import get_loss` becomes `get_loss = graphed.wrap_loss(model, get_loss)`)
        loss_fn = graphed.wrap_loss(model, total_loss) if args.wrap_loss else total_loss

    seg = {"forward": 0.0, "loss": 0.0, "backward": 0.0, "optimizer": 0.0}

    def body(data_dict):
        t = [time.perf_counter()]
        dd = model(data_dict); t.append(time.perf_counter())
        loss = loss_fn(dd); t.append(time.perf_counter())
        opt.zero_grad(set_to_none=True)
        loss.backward(); t.append(time.perf_counter())
        opt.step(); t.append(time.perf_counter())
        for k, a, b in zip(seg, t[:-1], t[1:]):
            seg[k] += (b - a) * 1e3
        return loss

    def loader(n):
        ld = _StaticLoader(batch, n)
        return graphed.prefetch_loader(model, ld) if prefetch else ld
    for data_dict in loader(max(warmup, 5)):
        body(data_dict)
    for k in seg:
        seg[k] = 0.0
    if use_graph and trace:
        model._graphed.host_times = {}
        model._graphed.phase_events = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = []
    h0 = time.perf_counter()
    for i, data_dict in enumerate(loader(steps)):
        if state0 is not None and i == steps - 1:   # (see restore_initial_state; not timed, the steps before it are)
            torch.cuda.synchronize()
            r0 = time.perf_counter()
            restore_initial_state(model, opt, state0)
            t0 += time.perf_counter() - r0
            h0 += time.perf_counter() - r0
        loss = body(data_dict)
        host.append((time.perf_counter() - h0) * 1e3)
        h0 = time.perf_counter()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dump_dir:
        dump_outputs(dump_dir, model, loss)
    assert torch.isfinite(loss).item()
    print("reference loop, host-side time per step: %.2f ms  (%s)" % (sum(host) / len(host), "  ".join("%s %.2f" % (k, v / steps) for k, v in seg.items())),
          file=sys.stderr)
    if use_graph and model._graphed.phase_events:
        print("reference loop, GPU ms since the step's first launch, per graph [start -> end on its stream]: " +
              "  ".join("%s %.1f->%.1f" % (k, a, b) for k, (a, b) in model._graphed.phase_gpu_ms().items()), file=sys.stderr)
    if use_graph and model._graphed.host_times:
        print("reference loop, host ms per graph launch: " + "  ".join("%s %.2f" % (k, sum(v) / len(v)) for k, v in model._graphed.host_times.items()),
              file=sys.stderr)
    runner = getattr(model, "_graphed", None)
    n_graphs = (len(runner.graphs) + 2 * len(runner.losses) + len(runner.opt_graphs)) if (use_graph and runner.graphs) else 0
    res = {"ms_per_step": round(dt / steps * 1e3, 3), "samples_per_s": round(args.batch * steps / dt, 3), "steps": steps,
           "loop": "reference: for data_dict in loader: model(data_dict) -> loss -> zero_grad -> backward -> optimizer.step, "
                   "body unchanged (lib/solver.py:463-595)",
           "hip_graph": bool(use_graph),
           "schedule": (("graphed.enable: %d graphs on 2 streams behind the module API (forward, backward%s%s%s)"
                         % (n_graphs, ", loss (graphed.wrap_loss)" if args.wrap_loss else "; loss eager",
                            ", optimizer (graphed.wrap_optimizer)" if runner.opt_graphs else "; optimizer eager",
                            ", next batch's FPS / ball query / three-NN under the fusion (graphed.prefetch_loader)" if prefetch else ""))
                        if use_graph else "eager, kernel by kernel"),
           "host_ms_per_step": round(sum(host) / len(host), 2)}
    if use_graph:
        graphed.disable(model)
    return res


def reference_loop(args, model, batch, dev, use_graph):
    """`--loop reference`: ONLY the drop-in loop, as its own JSON line"""
    res = run_reference_loop(args, model, batch, dev, use_graph, args.steps, args.warmup,
                             trace=os.environ.get("BQ_PIPE_TRACE") == "1", dump_dir=args.dump_outputs)
    out = {"metric": "train samples/s (%dk-pt scene + %d^2 view, bs%d)" % (args.points // 1000, args.image, args.batch),
           "value": res["samples_per_s"], "unit": "samples/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": WORKLOADS["c5" if args.workload == "c5" else "c3"], "global_batch": args.batch,
                      "points": args.points, "c_in": args.cin, "image": args.image, "parallelism": "dp1",
                      "loop": res["loop"], "hip_graph": bool(use_graph), "schedule": res["schedule"]},
           "host_ms_per_step": res["host_ms_per_step"],
           "note": "NOT the headline line: the drop-in loop of INTEGRATION.md §3 (the headline is --loop phased)"}
    print(json.dumps(_json_safe(out)))


def det_bwd_roofline(args, dev):
    """The fused SharedMLP backward (csrc/detbwd.hip) at SA1's three layer shapes of this configuration: algorithmic HBM bytes
    (operands read once, dX written once) over the live launch duration (HIP events on the launch stream, median of 7), next to
    the counter bytes of the committed PMC passes (profiles/r06_det_bwd_pmc.txt, taken at B = 16 x 2048 x 64 rows)."""
    import torch
    from bridgeqa_amd import _ext
    R = args.batch * 2048 * 64
    shapes = (("SA1 layer 0 (136 -> 64, no dX)", 136, 64, False, False), ("SA1 layer 1 (64 -> 64)", 64, 64, False, True),
              ("SA1 layer 2 (64 -> 128, max over 64)", 64, 128, True, True))
    per, tot_b, tot_ms = [], 0.0, 0.0
    st = torch.cuda.current_stream(dev)
    for name, ldx, N, pool, need_dx in shapes:
        if R * max(ldx, N) * 2 >= (1 << 31) - (1 << 20) or not _ext.sa_bwd_supported(ldx, N, 64, pool, need_dx):
            return None
        x = torch.randn(R, ldx, device=dev).to(torch.bfloat16)
        y_raw = torch.randn(R, N, device=dev).to(torch.bfloat16)
        dout = torch.randn(R // 64 if pool else R, N, device=dev).to(torch.bfloat16)
        arg = torch.randint(0, 64, (R // 64, N), device=dev, dtype=torch.uint8) if pool else None
        w = (torch.randn(N, ((ldx + 63) // 64) * 64, device=dev) * 0.05).to(torch.bfloat16)
        stats = torch.stack([torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev) * 0.1, torch.randn(N, device=dev) * 0.1,
                             torch.rand(N, device=dev) + 0.5, torch.zeros(N, device=dev)])
        dgb = _ext.bn_bwd_reduce(dout, y_raw, stats, 64, True, pool, arg)
        ts = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _ext.sa_bwd_fused(x, y_raw, dout, arg, w, stats, dgb, 64, True, pool, need_dx)
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = sorted(ts[2:])[len(ts[2:]) // 2]
        alg = R * 2.0 * (ldx + N + (0 if pool else N) + (ldx if need_dx else 0)) + (R // 64 * N * 3.0 if pool else 0.0)
        per.append({"layer": name, "rows": R, "ms": round(ms, 4), "algorithmic_bytes": alg,
                    "GB/s": round(alg / (ms * 1e-3) / 1e9, 1)})
        tot_b += alg
        tot_ms += ms
        del x, y_raw, dout, arg
    return {"kernel": "bq::sa_bwd_kernel (csrc/detbwd.hip): BatchNorm input gradient formed in LDS, dX and dW of a SharedMLP "
                      "layer from one pass over its activations; the three layers of SA1", "bound": "hbm",
            "achieved": round(tot_b / (tot_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(tot_b / (tot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "ms_total": round(tot_ms, 4), "per_layer": per,
            "traffic_from_profile": "profiles/r06_det_bwd_pmc.txt (2 x FETCH_SIZE + WRITE_SIZE per launch: 1125 / 1082 / 1103 MB "
                                    "for 1107 / 1074 / 1086 MB of algorithmic bytes at B = 16)",
            "timed_on": "dedicated launches after the timed region, HIP events on the launch stream, median of 7"}



def _fps_pmc():
    """physical HBM traffic of SA1's FPS launch from the committed counter passes (tools/run_r5_profiles.sh), or None"""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "r06_fps_pmc.json")))
    except (OSError, ValueError):
        return None


def ballquery_roofline(args, ops, alone_ms, alone_bg_ms, phased):
    """SA1's ball query (north_star names the op): SURVEY §8d's streaming-equivalent 12 N M B bytes per launch -- what the
    reference's kernel streams (every centre reads every point) -- over the launch's duration in the step and alone, next to
    the physical HBM traffic of the committed counter pass (the scene is L2-resident: 16 x 480 KB).  Like roofline_fps this
    is NOT a physical bandwidth: the kernel is bound by its vector instructions (kernel table)."""
    B, N, M = args.batch, args.points, 2048
    alg = 12.0 * N * M * B
    ms, cnt = ops.get(("ball_query", (B, M, 3)), (float("nan"), 0))
    eq = lambda t: round(alg / (t * 1e-3) / 1e9, 1) if t == t and t > 0 else None
    pmc = None
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", "r06_ballquery_pmc.json")))
        if (pmc.get("B"), pmc.get("N"), pmc.get("M")) != (B, N, M):
            pmc = None   # (taken at another shape: not this run's traffic)
    except (OSError, ValueError):
        pass
    return {"kernel": "bq::grid_box_kernel + grid_cellid_kernel + grid_chunk_kernel + bq::ball_query_grid_kernel (csrc/ball_query_grid.hip: "
                      "a uniform grid leaves ~100 candidate points per centre instead of all N; index-exact), SA1: %d centres x %d points, radius 0.2, "
                      "nsample 64, B=%d" % (M, N, B),
            "bound": "hbm", "convention": "streaming-equivalent (SURVEY §8d): 12*N*M*B bytes per launch = what the reference's "
                                          "exhaustive kernel streams -- this kernel SKIPS ~99 % of them, so `frac` far above 1 is the "
                                          "pruning factor, not a bandwidth; physical traffic: `traffic`",
            "algorithmic_bytes_per_launch": alg, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "achieved": eq(ms), "frac": round(eq(ms) / HBM_PEAK_GBS, 4) if eq(ms) else None, "ms_per_launch": round(ms, 4),
            "launches_timed": cnt,
            "timed_on": ("the timed steps: the geometry phase of the NEXT batch, running under the fusion chain"
                         if phased else "eager re-run after the graph replay"),
            "alone": {"ms_per_launch": round(alone_ms, 4), "achieved": eq(alone_ms),
                      "frac": round(eq(alone_ms) / HBM_PEAK_GBS, 4) if eq(alone_ms) else None,
                      "background_grid_ms_per_launch": round(alone_bg_ms, 4),
                      "exhaustive_scan_ms_per_launch": round(alone_bg_ms, 4),
                      "note": "5 back-to-back launches after the timed region, idle GPU; exhaustive_scan = bq_ball_query (the "
                              "wave-per-centre-pair scan of rounds 3-4) on the same inputs"},
            "traffic": pmc}


def _json_safe(x):
    """NaN / inf -> null: the bench line must be strict JSON"""
    if isinstance(x, float):
        return x if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {k: _json_safe(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_json_safe(v) for v in x]
    return x


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N fresh ranks (one process per GPU, RCCL) through
    torch.distributed.run as a CHILD process, before this process has made any GPU call, and exit with its code.  Never
    silently runs fewer GPUs than asked for: too few devices is an error."""
    import socket
    import subprocess
    have = torch.cuda.device_count()   # (counts devices without initialising the GPU on this image)
    if have < args.gpus and not args.share_device:
        sys.stderr.write("bench.py: --gpus %d requested, %d visible device(s): refusing to run fewer ranks\n"
                         % (args.gpus, have))
        sys.exit(2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (python -m torch.distributed.run "
                         "--nproc-per-node %d ... bench.py --gpus %d)\n" % (args.gpus, world, args.gpus, args.gpus))
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU product path)"
    if args.share_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1 or (args.dp_path and "RANK" in os.environ):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=args.backend, init_method="env://")
    workload = "c3" if args.workload in ("auto", "c5") else args.workload   # (c5 = the c3 path at the large sizes)

    from bridgeqa_amd import _ext, fusion_ops
    if workload == "c3" and args.dtype != "bf16":
        raise SystemExit("bench.py: workload c3 is defined in bf16 (BASELINE.json configs[2])")
    if args.dtype == "bf16":
        fusion_ops.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model(workload, args.cin, args.image).to(dev)
    state0 = initial_state(model) if args.dump_outputs else None
    dp = world > 1 or args.dp_path  # data-parallel structure: graph(fwd+bwd) -> flat bf16 all-reduce -> fused AdamW
    use_graph = args.graph in ("on", "auto")
    batch = make_batch(args, workload, args.batch, 42 + rank, dev)
    side = torch.cuda.Stream()
    graphed = False

    if args.loop == "reference":
        if workload != "c3" or world > 1:
            raise SystemExit("bench.py: --loop reference is the single-GPU c3 / c5 drop-in loop")
        return reference_loop(args, model, batch, dev, use_graph)
    phased = workload == "c3"  # one HIP graph per phase on two streams (bridgeqa_amd/pipeline.py); c2: one graph
    pipe = None
    if phased:
        # ---- single GPU, c3: one HIP graph per phase, image / fusion chain on one stream, detector on a second,
        # high-priority one (bridgeqa_amd/pipeline.py) -------------------------------------------------------
        from bridgeqa_amd.pipeline import PhasedTrainStep
        # one HIP launch for all parameters, bf16 operand copies written in the same pass (csrc/adamw.hip); the
        # clip_grad_value_(1.0) of the reference's step (lib/solver.py:407-409) happens inside the update kernel
        from bridgeqa_amd.optim import FusedAdamW
        opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=1e-5, grad_clip_value=1.0)
        # the geometry phase (FPS / ball query of the next batch) stays eager so that the roofline kernel is timed
        # with HIP events INSIDE the timed steps, on the stream it is launched on
        # next_batch=batch: the benchmark replays ONE static synthetic batch, so "the next step's point clouds" are the
        # same buffers (a training loop passes the buffers its loader fills one step ahead)
        bb = None
        if dp:
            # data parallel: the image backward in three block ranges (their gradient groups travel under the ranges that
            # follow; only the last one is exposed) and DDP's per-step buffer broadcast (scripts/train.py:346-347)
            from bridgeqa_amd.ddp import BufferBroadcaster
            bb = BufferBroadcaster(model)
            bb.force = args.dp_path
        pipe = PhasedTrainStep(model, batch, det_loss, fusion_loss, opt, use_graphs=use_graph, next_batch=batch,
                               eager_phases=("geometry",), image_bwd_splits=3 if dp else 1, buffer_broadcaster=bb,
                               text_prologue=args.text_prologue)
        eager_step = pipe.eager_step
        reducers = {}
        if dp:
            # data parallel: each phase's gradients are packed to bf16, all-reduced over RCCL on a communication
            # stream as soon as that phase's backward has finished, unpacked, and the optimizer waits for all three
            from bridgeqa_amd.ddp import PackedGradReducer, broadcast_parameters
            broadcast_parameters(model)

            def make_reducer(ps):
                r = PackedGradReducer(ps, comm_dtype=torch.bfloat16, algo=args.grad_exchange)
                r.force = args.dp_path
                return r
            reducers = pipe.attach_reducers(make_reducer)
    geometry_ahead = None
    if not phased and not args.no_geometry_prefetch:
        # ---- c2: the sampling / grouping indices (FPS, ball query, three-NN: a latency chain on B workgroups, a quarter
        # of the step) depend on the point coordinates only, so those of the NEXT batch are computed on a second stream
        # while this step runs -- what pipeline.PhasedTrainStep does for c3 (next_batch = the static synthetic batch here; a
        # training loop passes the buffers its loader fills one step ahead).  The captured step reads `geo_cur`.
        bbone = model.detection_backbone
        s_geo = torch.cuda.Stream()
        with torch.no_grad():
            geo0 = bbone.precompute_geometry(batch["point_clouds"])
        geo_next = {k: v.clone() for k, v in geo0.items()}
        geo_cur = {k: v.clone() for k, v in geo0.items()}
        batch = dict(batch)
        batch["geometry"] = geo_cur
        e_geo, e_cur = torch.cuda.Event(), torch.cuda.Event()
        e_geo.record(torch.cuda.current_stream())

        def geometry_ahead(stage):
            # stage 0 (before the step's graph is launched): next -> cur.  stage 1 (AFTER it is launched: the host issues
            # these ~60 eager launches while the graph already runs): the following batch's indices on the second stream
            if stage == 0:
                cur_s = torch.cuda.current_stream()
                cur_s.wait_event(e_geo)              # the indices computed while the previous step ran
                for k in geo_cur:
                    geo_cur[k].copy_(geo_next[k])
                e_cur.record(cur_s)
                return
            s_geo.wait_event(e_cur)                  # (geo_next may be refilled now)
            with torch.cuda.stream(s_geo):
                if geo_graph[0] is not None:
                    geo_graph[0].replay()            # (one launch: ~60 eager launches per step made the step host-sensitive)
                else:
                    geo_body()
                e_geo.record(s_geo)

        def geo_body():
            from bridgeqa_amd.pointnet2_utils import background_geometry
            with torch.no_grad(), background_geometry():
                gnew = bbone.precompute_geometry(batch["point_clouds"])
                for k in geo_next:
                    geo_next[k].copy_(gnew[k])
        geo_graph = [None]
        if use_graph:
            with torch.cuda.stream(s_geo):
                for _ in range(2):
                    geo_body()
            torch.cuda.synchronize()
            gg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gg, stream=s_geo):
                geo_body()
            torch.cuda.synchronize()
            geo_graph[0] = gg
    if phased:
        pass
    elif not dp:
        # ---- single GPU: forward + backward + fused AdamW replayed from ONE HIP graph -----------------------
        # (fused multi-tensor AdamW; NB the foreach implementation under capture makes hipStreamEndCapture segfault)
        opt = torch.optim.AdamW(model.parameters(), lr=5e-4, weight_decay=1e-5, fused=True, capturable=use_graph)

        def eager_step():
            # grads start as None: autograd then hands each gradient tensor over without a zero-fill + add per
            # parameter (under capture the buffers come from the graph's private pool at fixed addresses)
            opt.zero_grad(set_to_none=True)
            loss = total_loss(model(dict(batch)))
            loss.backward()
            opt.step()
            return loss
        graph_body = eager_step
        after_replay = lambda: None
    else:
        # ---- data parallel, detector-only workload: the forward+backward is one HIP graph without collectives, then ONE
        # packed all-reduce of every used gradient over RCCL (bridgeqa_amd/ddp.py), then fused AdamW
        from bridgeqa_amd.ddp import PackedGradReducer, broadcast_parameters, used_parameters
        broadcast_parameters(model)

        def dry():
            for p in model.parameters():
                p.grad = None
            total_loss(model(dict(batch))).backward()
        with torch.cuda.stream(side):
            used = used_parameters(model, dry)
        torch.cuda.synchronize()
        reducer = PackedGradReducer(used, comm_dtype=torch.bfloat16, algo=args.grad_exchange)
        reducer.force = args.dp_path
        opt = torch.optim.AdamW(used, lr=5e-4, weight_decay=1e-5, fused=True)

        def graph_body():
            for p in used:
                p.grad = None
            loss = total_loss(model(dict(batch)))
            loss.backward()
            return loss

        def after_replay():
            reducer.all_reduce()
            opt.step()

        def eager_step():
            loss = graph_body()
            after_replay()
            return loss

    if phased:
        pipe.capture(warmup=max(args.warmup, 3 if use_graph else 0))
        graphed = use_graph

        def step():
            return pipe.step()
        for _ in range(2):
            step()
        if os.environ.get("BQ_PIPE_TRACE") == "1":
            pipe.host_times = {}
            pipe.phase_events = {}
        if reducers:   # per-group communication time and the exposed part of it, measured inside the timed steps
            pipe.comm_stall = []
            for r_ in reducers.values():
                r_.timing = []
        use_graph = False  # (the single-graph capture below is the other schedule)
    else:
        step = eager_step
        if geometry_ahead is not None:
            # --graph off: the same schedule kernel by kernel (stage 0: next -> cur, the step, stage 1: the following
            # batch's indices on the second stream) -- without this the timed region would consume indices computed once
            # before it
            def step():
                geometry_ahead(0)
                loss_ = eager_step()
                geometry_ahead(1)
                return loss_
    # Every eager step before a capture runs on the SAME side stream: autograd's AccumulateGrad nodes remember the
    # stream they were created on, and nodes born on the default stream make hipStreamEndCapture segfault (ROCm 7).
    if not phased:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(args.warmup, 3 if use_graph else 0)):
                eager_step()
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if use_graph:
        # The step is launch-bound in places (thousands of short kernels): capture it ONCE and replay.  Inputs are
        # static device buffers.
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = graph_body()
        torch.cuda.synchronize()

        def step():
            if geometry_ahead is not None:
                geometry_ahead(0)
            g.replay()
            after_replay()
            if geometry_ahead is not None:
                geometry_ahead(1)
            return static_loss
        graphed = True
        for _ in range(2):
            step()
    # (wrapped in every run, so that a plain run times the same launches as a --full one, which reports them as op_ms)
    timer = OpTimer()
    timer.wrap(_ext, ["furthest_point_sampling", "ball_query", "group_concat", "group_concat_grad"])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    host_ms = 0.0
    host_each = []
    for i in range(args.steps):
        if state0 is not None and i == args.steps - 1:
            torch.cuda.synchronize()   # (the steps before it stay on the clock; the restore itself is not timed)
            r0 = time.perf_counter()
            restore_initial_state(model, opt, state0)
            t0 += time.perf_counter() - r0
        h0 = time.perf_counter()
        loss = step()
        host_each.append((time.perf_counter() - h0) * 1e3)
        host_ms += host_each[-1]
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss)   # (before the eager re-run below, which steps the optimizer again)
    # A plain run launches nothing more on the GPU (a data-parallel run still checks its replicas, below).  What follows up to
    # the reference's loop and the CPU baseline is --full only: per-kernel timings from launches of their own.
    if args.full and graphed:
        # a replayed graph runs no Python, so the per-kernel HIP events are taken on an eager re-run of the same
        # step (same kernels, same stream) right after the timed region; it is not part of `value`
        if phased:
            pass  # the geometry phase was launched eagerly inside the timed steps: its kernels are already timed
        else:
            with torch.cuda.stream(side):
                for it in range(min(args.steps, 3) + 1):
                    if it == 1:
                        torch.cuda.synchronize()
                        del timer.records[:]   # (the first eager pass after the replays re-grows the eager allocator's pool)
                    if geometry_ahead is not None:
                        geo_body()   # (the prefetched indices come from a replayed graph too: the same launches, eagerly)
                    eager_step()
        torch.cuda.synchronize()
    timer.unwrap()
    # the same FPS launch with nothing else on the GPU (in the step it runs UNDER the image encoder's GEMMs)
    fps_alone_ms = float("nan")
    if args.full and rank == 0:
        xyz_alone = batch["point_clouds"][..., :3].contiguous()
        _ext.furthest_point_sampling(xyz_alone, 2048)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(5):
            _ext.furthest_point_sampling(xyz_alone, 2048)
        ev1.record()
        torch.cuda.synchronize()
        fps_alone_ms = ev0.elapsed_time(ev1) / 5
    # SA1's ball query (2048 centres x all points, radius 0.2, 64 samples) alone: the full grid and the background grid
    bq_alone_ms = bq_alone_bg_ms = float("nan")
    if args.full and rank == 0:
        ctr = xyz_alone[:, :2048].contiguous()   # (any 2048 points serve as centres for the timing: the scan is exhaustive)
        for bg in (False, True):   # (bg: the exhaustive scan of rounds 3-4 for comparison -- the grid withdrawn)
            prev_min = _ext.BALL_QUERY_GRID_MIN_N[0]
            if bg:
                _ext.BALL_QUERY_GRID_MIN_N[0] = 1 << 30
            _ext.ball_query(ctr, xyz_alone, 0.2, 64)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(5):
                _ext.ball_query(ctr, xyz_alone, 0.2, 64)
            ev1.record()
            torch.cuda.synchronize()
            _ext.BALL_QUERY_GRID_MIN_N[0] = prev_min
            if bg:
                bq_alone_bg_ms = ev0.elapsed_time(ev1) / 5
            else:
                bq_alone_ms = ev0.elapsed_time(ev1) / 5
    replicas_in_sync = None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
        # data parallel invariant: after the same number of steps every rank holds the same PARAMETERS (reference: DDP's
        # gradient averaging, scripts/train.py:346-347) -- one checksum per rank.  (Buffers -- BatchNorm running statistics
        # -- legitimately differ between a step's forward and the broadcast that opens the next one, as under DDP.)
        # (one checksum PER PARAMETER, two moments each: a single global sum |p| would not see compensating differences)
        with torch.no_grad():
            cs = torch.stack([torch.stack((p.detach().double().sum(), p.detach().double().abs().sum()))
                              for p in model.parameters()]).reshape(-1)
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_in_sync = bool(torch.equal(lo, hi))
        if rank == 0 and not replicas_in_sync:
            bad = (lo != hi).reshape(-1, 2).any(1).nonzero().reshape(-1).tolist()
            names = [n for n, _ in model.named_parameters()]
            print("bench.py: %d parameter(s) differ between ranks, first: %s" % (len(bad), [names[i] for i in bad[:5]]),
                  file=sys.stderr)
    assert torch.isfinite(loss).item()
    if rank == 0 and pipe is not None and pipe.phase_events:
        print("GPU ms since the step's first launch, per phase [start -> end on its stream]: " +
              "  ".join("%s %.1f->%.1f" % (k, a, b) for k, (a, b) in pipe.phase_gpu_ms().items()), file=sys.stderr)
    if rank == 0 and pipe is not None and pipe.host_times:
        print("host ms per graph launch: " + "  ".join("%s %.1f" % (k, sum(v) / len(v)) for k, v in pipe.host_times.items()),
              file=sys.stderr)
    if rank == 0:
        print("host-side launch time per step: %.2f ms  [%s]" % (host_ms / args.steps, " ".join("%.1f" % h for h in host_each)), file=sys.stderr)

    # --full: the same model behind the reference's UNCHANGED loop, timed in this process right after the headline (INTEGRATION.md
    # section 3a; before the CPU baseline, whose 32 OpenMP threads keep spinning on the host): the phased step's graphs are
    # dropped first
    loop_ref_res, n_phase_graphs = None, (len(pipe.graphs or ()) if pipe is not None else 0)
    if (args.full and rank == 0 and phased and world == 1 and not args.no_loop_reference and args.workload != "c5"
            and not dp):
        pipe.graphs, pipe._state = None, {}
        step = None
        pipe = None
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        try:
            loop_ref_res = run_reference_loop(args, model, batch, dev, args.graph in ("on", "auto"), args.steps, args.warmup,
                                              trace=os.environ.get("BQ_PIPE_TRACE") == "1")
        except Exception as e:    # (the headline line must not be lost to the second measurement)
            loop_ref_res = {"error": "%s: %s" % (type(e).__name__, e)}

    if rank == 0:
        out = {
            "metric": ("train samples/s (%dk-pt scene + %d^2 view, bs%d)" % (args.points // 1000, args.image, args.batch)
                       if workload == "c3" else "train samples/s (40k-pt scene, DET stage only, bs16)"),
            "value": round(args.batch * world * args.steps / dt, 3),
            "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": WORKLOADS["c5" if args.workload == "c5" else workload], "global_batch": args.batch * world,
                       "points": args.points,
                       "c_in": args.cin, "image": args.image if workload == "c3" else None,
                       "parallelism": "dp%d" % world, "hip_graph": graphed,
                       "schedule": (("phased: %d graphs on 2 streams" % n_phase_graphs) if phased else
                                    ("single graph + the next batch's sampling / grouping indices on a second stream"
                                     if geometry_ahead is not None else "single graph")),
                       "grad_exchange": (("per-phase packed bf16 all-reduce on a comm stream, %d MB on the wire"
                                          % (sum(r.nbytes_on_wire() for r in reducers.values()) >> 20)) if phased
                                         else ("one packed bf16 all-reduce after the fwd+bwd graph, %d MB on the wire"
                                               % (reducer.nbytes_on_wire() >> 20))) if dp else None},
        }
        if args.full:
            ops = timer.summary()
            # dominant native kernel: SA1 furthest point sampling; algorithmic bytes 20*N*(m-1) per scene
            key = ("furthest_point_sampling", (args.batch, args.points, 3))
            fps_ms, _ = ops.get(key, (float("nan"), 0))
            alg = 20.0 * args.points * (2048 - 1) * args.batch
            achieved = alg / (fps_ms * 1e-3) / 1e9
            out.update({
                "roofline": None,      # filled below: the dominant dense kernel (MFMA GEMM)
                "roofline_fps": {"kernel": "fps (SA1 %d->2048), csrc/fps_bucket.hip" % args.points, "bound": "hbm",
                                 "convention": "streaming-equivalent (SURVEY §8d), NOT physical traffic: 20*N*(m-1) bytes per "
                                               "scene = what the reference's kernel streams; this kernel prunes ~41x of it "
                                               "and is latency-bound (serial arg-max rounds)",
                                 "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": round(achieved / HBM_PEAK_GBS, 4), "ms_per_launch": round(fps_ms, 4),
                                 "rounds": 2047, "us_per_round": round(fps_ms * 1e3 / 2047, 3),
                                 "floor_us_per_round": 0.5, "floor_frac": round(0.5 / (fps_ms * 1e3 / 2047), 3),
                                 "traffic_from_profile": _fps_pmc() if (args.points == 40000 and args.batch == 16) else None,
                                 "timed_on": ("the timed steps (geometry phase launched eagerly between the graph replays)"
                                              if phased else "eager re-run after the graph replay" if graphed
                                              else "the timed steps"),
                                 "algorithmic_bytes_per_launch": alg,
                                 "alone": {"ms_per_launch": round(fps_alone_ms, 4),
                                           "achieved": round(alg / (fps_alone_ms * 1e-3) / 1e9, 1),
                                           "frac": round(alg / (fps_alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                           "note": "5 back-to-back launches after the timed region, idle GPU"}},
                "roofline_ballquery": ballquery_roofline(args, ops, bq_alone_ms, bq_alone_bg_ms, phased),
                "op_ms": {"%s%s" % (k[0], list(k[1])): round(v[0], 4) for k, v in sorted(ops.items())},
                "path_roofline": (lambda tm, det: {"t_min_ms": round(tm, 3), "frac": round(tm / (dt / args.steps * 1e3), 4),
                                                   **det})(*path_roofline(args, workload)),
            })
            if workload == "c3":
                per, tot_f, tot_ms, traffic, prof_frac = gemm_roofline(args, dev)
                out["roofline"] = {"kernel": "bq::gemm128_kernel (csrc/gemm_mid.hip: forward / input-gradient forms, 256x128 tiles, "
                                             "persistent, 2 workgroups per CU) + bq::gemm256_kernel (csrc/gemm.hip: weight gradients and, since round 6, the "
                                             "forward / dX launches with a contraction >= 2304: fc2 forward, dX through fc1 and qkv): "
                                             "the 8 launches of one ViT block (forward + dX, with the epilogues the step uses) + "
                                             "the grouped dW launch of all 12 blocks", "bound": "mfma",
                                   "achieved": round(tot_f / tot_ms / 1e9, 1), "peak": 2500.0, "unit": "TFLOP/s",
                                   "frac": round(tot_f / tot_ms / 1e9 / 2500.0, 4),
                                   "frac_uses": "sum of the live HIP-event medians below (per_gemm[].us)",
                                   "from_profile_durations": prof_frac,
                                   "traffic": traffic,
                                   "algorithmic_flops": tot_f, "ms_total": round(tot_ms, 4), "per_gemm": per,
                                   "timed_on": "dedicated launches after the timed region, HIP events on the launch stream, "
                                               "median of 10 (inside the step the same kernels replay from HIP graphs; the "
                                               "in-step averages come from profiles/r06_c3_kernel_stats.csv, the counters from "
                                               "profiles/r06_gemm_pmc.jsonl; both only at M = 16400, the shape they were taken at)"}
                out["roofline_attn"] = attn_roofline(args, dev)
            else:
                out["roofline"] = out["roofline_fps"]
            if world == 1 and args.workload != "c5":
                out["roofline_det_bwd"] = det_bwd_roofline(args, dev)
            if world == 1 and not args.no_cpu_baseline and args.workload != "c5":   # (c3 is the headline: its baseline is the one reported)
                out["cpu_baseline"] = cpu_baseline(args, workload)
            if loop_ref_res is not None:
                out["loop_reference"] = loop_ref_res
        if replicas_in_sync is not None:
            out["replicas_in_sync"] = replicas_in_sync
        if pipe is not None and reducers:
            out["comm"] = pipe.comm_report()
        out["config"]["batches"] = "one static synthetic batch replayed every step (the geometry is recomputed every step)"
        if args.share_device:
            out["data"] += " [--share-device validation run: all ranks on one GPU, throughput not meaningful]"
        print(json.dumps(_json_safe(out)))
    if dist.is_initialized():
        dist.destroy_process_group()
    if replicas_in_sync is False:
        sys.exit(3)   # (diverged replicas must fail a scaling / CI run, not only print -- ADVICE r3)


if __name__ == "__main__":
    main()
