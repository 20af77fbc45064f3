"""bench.py's launch contract: `--gpus N` is never silently a one-GPU run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_gpus_n_without_enough_devices_fails_loudly():
    import torch
    if torch.cuda.device_count() >= 2:
        return  # (a multi-GPU box would start the ranks; the refusal is what is tested here)
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 2 and "refusing to run fewer ranks" in r.stderr, (r.returncode, r.stderr[-400:])
    assert r.stdout.strip() == ""   # no JSON line that could be mistaken for a result


def test_gpus_n_must_equal_world_size():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr, (r.returncode, r.stderr[-400:])


def test_steps_below_one_is_refused():
    r = _run(["--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr, (r.returncode, r.stderr[-400:])


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_sample_is_fixed_aligned_and_bounded(tmp_path):
    """--dump-outputs on a model larger than the sample: the same positions in every run and for parameters and gradients
    alike (a parameter without a gradient dumps zeros), float32 / float64 only, 64 MB at most"""
    import numpy as np
    import torch
    bench = _bench()
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3000, 2000), torch.nn.BatchNorm1d(2000))
    loss = m(torch.randn(4, 3000)).square().mean()
    loss.backward()
    m[1].weight.grad = None
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, loss)
    names = {"loss", "parameters", "gradients", "buffers"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in names}
    assert all(a[n].dtype in (np.float32, np.float64) for n in names)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES
    assert all(np.array_equal(a[n], b[n]) for n in names)
    assert a["loss"][0] == loss.item() and a["parameters"].size == bench.DUMP_SAMPLE
    params = list(m.parameters())
    total = sum(p.numel() for p in params)
    pos = torch.randint(0, total, (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(1)).sort().values
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
    assert np.array_equal(a["parameters"], flat_p[pos].numpy()) and np.array_equal(a["gradients"], flat_g[pos].numpy())
    # below the sample size every element is written, in order
    flat_b = torch.cat([t.reshape(-1).float() for t in (m[1].running_mean, m[1].running_var)])
    assert np.array_equal(a["buffers"], flat_b.numpy())


def test_full_is_off_by_default(monkeypatch):
    """a plain run measures the headline alone; what takes runs of its own waits for --full"""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True
