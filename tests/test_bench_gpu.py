"""bench.py's N > 1 control flow on a ONE-GPU box: two ranks that share cuda:0 over gloo (RCCL refuses two ranks on one
device).  What runs is what `--gpus 2` runs on two GPUs -- per-rank synthetic batches, the phased step with its per-phase
packed gradient groups (the image backward in three block ranges), DDP's buffer broadcast, fused AdamW -- except the wire.
Checked: one JSON line, n_gpus = 2, finite throughput, and the data-parallel invariant: both ranks hold the same parameters
and buffers after the steps (reference: DistributedDataParallel, scripts/train.py:346-347)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("workload,extra", [("c3", ["--batch", "2", "--points", "4096", "--image", "128"]),
                                            ("c3", ["--batch", "2", "--points", "4096", "--image", "128", "--grad-exchange",
                                                    "reduce_scatter"]),
                                            ("c2", ["--batch", "2", "--points", "4096"])])
def test_two_ranks_sharing_one_device_stay_in_sync(workload, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device",
                        "--workload", workload, "--steps", "3", "--warmup", "2", "--no-cpu-baseline"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["scaling"] == "weak"
    assert out["replicas_in_sync"] is True, r.stderr[-1500:]
    assert "validation run" in out["data"]
    if workload == "c3":
        # per-group communication time and its exposed part, from events on the communication / main stream: the fields the
        # first real multi-GPU run turns DESIGN §6's predicted table into (their VALUES mean nothing on a shared device)
        comm = out["comm"]
        assert set(comm["groups"]) == {"fusion", "det", "image_0", "image_1", "image_2"}
        assert all(g["ms"] is not None and g["ms"] > 0 and g["bytes_on_wire"] > 0 for g in comm["groups"].values())
        assert comm["exposed_ms"] is not None and comm["exposed_ms"] >= 0
        want = "reduce_scatter" if "reduce_scatter" in extra else "all_reduce"
        assert all(g["algo"] == want for g in comm["groups"].values())


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs on one GPU, the phased c3 step at a small size, twice: the JSON line reports the --steps asked for, DIR
    holds the last timed step's loss, parameters, gradients and buffers as finite float32 / float64 arrays (64 MB at most),
    and the two runs agree to rounding (the dumped step starts from the seeded state: bench.restore_initial_state)"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for run in ("a", "b"):
        out_dir = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c3", "--batch", "2",
                            "--points", "4096", "--image", "128", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                            "--no-loop-reference", "--dump-outputs", str(out_dir)],
                           env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == 3, r.stdout[-2000:]
        dumps.append({f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)})
    a, b = dumps
    assert set(a) == {"loss", "parameters", "gradients", "buffers"}
    assert all(x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert np.abs(a["gradients"]).max() > 0
    # measured: loss and buffers bit-identical, gradients within 3e-10 of their largest element, parameters within 1 ulp
    # (what is left are fp32 atomic sums)
    for n in a:
        x, y = a[n].astype(np.float64), b[n].astype(np.float64)
        assert x.shape == y.shape, n
        tol = 1e-6 * np.abs(x).max() + 1e-4 * np.abs(x)
        assert (np.abs(x - y) <= tol).all(), (n, float(np.abs(x - y).max()))


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_full_adds_the_rest():
    """a plain one-GPU run ends at its headline: the line carries metric / value / unit / ms_per_step and nothing that takes
    runs of its own; --full adds the rooflines, the per-kernel figures, the reference's loop and the CPU baseline (c3, small)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    moved = {"roofline", "roofline_fps", "roofline_ballquery", "roofline_attn", "roofline_det_bwd", "op_ms", "path_roofline",
             "loop_reference", "cpu_baseline"}
    for full in (False, True):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c3", "--batch", "2",
                            "--points", "4096", "--image", "128", "--steps", "3", "--warmup", "1"] + (["--full"] if full else []),
                           env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
        assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]
        if full:
            assert moved <= set(out), sorted(moved - set(out))
            assert "error" not in out["loop_reference"], out["loop_reference"]
            assert out["cpu_baseline"]["value"] > 0 and out["roofline"]["achieved"] > 0
        else:
            assert not moved & set(out), sorted(moved & set(out))
