"""The fused multi-tensor AdamW step (adamw_kernel, csrc/adamw.hip) held to the per-element fp64 bounds of tests/adamw_ref.py:
p', exp_avg and exp_avg_sq of every element, the bf16 shadows bit for bit, and every byte around the tensors.  Every comparison
is ONE step from the fp32 state the kernel itself was given (multi-step runs take each step's reference from the state the
kernel left), so no error compounds into the bound; `not (err <= tol)` fails, so NaN fails, and where the reference is NaN or
infinite the output must be the same.  tests/test_adamw_bound_cpu.py shows what the bound rejects.

The layout, value, exact, sweep and clamp batteries call _ext.adamw_multi directly on arenas the test lays out itself (record
layout of optim.FusedAdamW._build, canaries between the tensors); the wrapper battery goes through optim.FusedAdamW.

The largest |err| / bound per output kind is the last line the module prints (pytest -s).  On the MI355X: p 0.379, m 0.324,
v 0.290 over 1 160 688 elements each in 2.6 s.  The direct-launch batteries give p 0.362, m 0.315, v 0.290 -- the figures of
the CPU emulation to every printed digit, at t = 2 and 3 too, so the device powf uses no more of its term than a correctly
rounded one; the largest ratios come from the wrapper battery.  With the library of the commit before the clamp kept NaN,
exactly the three test_clamp_battery cases fail (a NaN gradient gave finite p', m', v' from a gradient of -clip with clipping,
m' = -inf and v' = +inf without) and the other 13 tests pass.
"""
import time

import numpy as np
import pytest
import torch

import adamw_ref as R

pytestmark = pytest.mark.gpu

KINDS = ("p", "m", "v")
_WORST, _COUNT = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print("\nAdamW battery: %.1f s; elements held per output kind: %s" % (
        time.time() - t0, "  ".join("%s %d" % (k, _COUNT.get(k, 0)) for k in KINDS)))
    print("largest |err| / bound per output kind: " + "  ".join("%s %.3g" % (k, _WORST.get(k, 0.0)) for k in KINDS))


@pytest.fixture(scope="module")
def ext(dev):
    from bridgeqa_amd import _ext
    assert _ext.ADAMW_TENSOR_BYTES == 56 == R.RECORD.itemsize and _ext.ADAMW_CHUNK == R.CHUNK
    return _ext


class _Hold:
    """collects the failures of one case; assert_ok() reports them all"""

    def __init__(self, name):
        self.name, self.fails, self.worst = name, [], dict.fromkeys(KINDS, 0.0)

    def __call__(self, kind, out, ref, tol, what):
        ratio, msg = R.excess(out, ref, tol)
        _WORST[kind] = max(_WORST.get(kind, 0.0), ratio)
        _COUNT[kind] = _COUNT.get(kind, 0) + ref.numel()
        self.worst[kind] = max(self.worst[kind], ratio)
        if msg:
            self.fails.append("%s %s %s: %s" % (self.name, what, kind, msg))

    def true(self, cond, msg):
        if not cond:
            self.fails.append("%s: %s" % (self.name, msg))

    def assert_ok(self):
        print("%s: largest |err| / bound %s" % (self.name, "  ".join("%s %.3g" % kv for kv in self.worst.items())))
        assert not self.fails, "\n".join(self.fails[:20] + ["(%d failures)" % len(self.fails)])


def _bits(x):
    return x.contiguous().view(torch.int32)


def _launch(dev, ext, L, shuffled=False, clip="launch", n_chunks=None):
    """lay the records of L out in five arenas full of canaries, run ONE adamw_multi launch over them, return (the arenas as
    uploaded, as the kernel left them, the tensors' places), all on the CPU"""
    recs = L["records"]
    at, size = R.place(recs)
    host = {k: torch.full((size[k],), R.CANARY32, dtype=torch.int32).view(torch.float32) for k in "pgmv"}
    host["s"] = torch.full((size["s"],), R.CANARY16, dtype=torch.int16).view(torch.bfloat16)
    for a, r in zip(at, recs):
        for k in "pgmv":
            host[k][a[k]:a[k] + r["n"]] = r[k]
    arena = {k: host[k].to(dev, copy=True) for k in "pgmvs"}
    assert all(arena[k].data_ptr() % 16 == 0 for k in "pgmvs")
    tab = np.zeros(len(recs), dtype=R.RECORD)
    for i, (a, r) in enumerate(zip(at, recs)):
        ptr = {k: arena[k].data_ptr() + 4 * a[k] for k in "pgmv"}
        tab[i] = (ptr["p"], ptr["g"], ptr["m"], ptr["v"], arena["s"].data_ptr() + 2 * a["s"] if a["s"] is not None else 0,
                  r["n"], r["lr"], r["wd"])
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    chunks = torch.from_numpy(R.chunk_list(recs, shuffled)[:n_chunks].copy()).to(dev).view(-1, 2)
    step = torch.tensor(float(L["t"]), dtype=torch.float32, device=dev)
    ext.adamw_multi(table, chunks, step, L["betas"][0], L["betas"][1], L["eps"], L["clip"] if clip == "launch" else clip)
    torch.cuda.synchronize()
    return host, {k: arena[k].cpu() for k in "pgmvs"}, at


def _hold_launch(hold, L, host, out, at):
    """every element of p', m', v' to the bound from the uploaded state; the shadow bit-equal to the stored p' rounded to
    nearest even (NaN where p' is NaN); lr = 0 leaves p bit-identical; g and every canary bitwise intact"""
    recs = L["records"]
    used = {k: torch.zeros(host[k].numel(), dtype=torch.bool) for k in "pgmvs"}
    for i, (a, r) in enumerate(zip(at, recs)):
        n = r["n"]
        what = "record %d (n %d, offsets %s, lr %g, wd %g)" % (i, n, {k: o for k, o in r["off"].items() if o}, r["lr"], r["wd"])
        ref = R.reference(r["p"], r["g"], r["m"], r["v"], L["t"], r["lr"], r["wd"], L["betas"], L["eps"], L["clip"])
        got = {k: out[k][a[k]:a[k] + n] for k in "pmv"}
        for k in "pmv":
            hold(k, got[k], ref[k], ref["tol_" + k], what)
            used[k][a[k]:a[k] + n] = True
        used["g"][a["g"]:a["g"] + n] = True
        if r["lr"] == 0:
            hold.true(torch.equal(_bits(got["p"]), _bits(r["p"])), what + ": lr = 0 did not leave p bit-identical")
        if a["s"] is not None:
            used["s"][a["s"]:a["s"] + n] = True
            s = out["s"][a["s"]:a["s"] + n]
            nan = torch.isnan(got["p"])
            hold.true(bool(torch.isnan(s.float()[nan]).all()), what + ": the shadow of a NaN parameter is not NaN")
            hold.true(torch.equal(R.bf16_bits(s)[~nan], R.bf16_bits(got["p"].to(torch.bfloat16))[~nan]),
                      what + ": the shadow is not the stored p' rounded to nearest even")
    hold.true(torch.equal(_bits(out["g"]), _bits(host["g"])), "the gradient arena changed")
    for k in "pgmv":
        hold.true(bool((_bits(out[k])[~used[k]] == R.CANARY32).all()), "a canary of the %s arena changed" % k)
    hold.true(bool((out["s"].view(torch.int16)[~used["s"]] == R.CANARY16).all()), "a canary of the shadow arena changed")


# ---- a. layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["table-order", "shuffled"])
def test_layout_battery(dev, ext, shuffled):
    """80 records in one launch: every length around the float4 tail and the 8192-element chunk boundary, each stream in turn
    1, 2 and 3 elements off its alignment at n % 4 == 0 (the kernel's `vec` predicate must send those down the scalar path),
    null shadows, three (lr, wd) pairs with wd = 0 and lr = 0, t = 7"""
    L = R.layout_launch()
    hold = _Hold("layout-%s" % ("shuffled" if shuffled else "ordered"))
    _hold_launch(hold, L, *_launch(dev, ext, L, shuffled))
    hold.assert_ok()


def test_no_chunks_is_no_launch_and_no_error(dev, ext):
    L = R.clamp_launch(1.0)
    host, out, _ = _launch(dev, ext, L, n_chunks=0)
    assert all(torch.equal(out[k].view(torch.int16), host[k].view(torch.int16)) for k in "pgmvs")


# ---- b. values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.value_launches(), ids=lambda L: "t%d-betas%g-%g" % ((L["t"],) + L["betas"]))
def test_value_battery(dev, ext, L):
    """gradients of 1, 1e-4, 1e-8, 1e-12 and 1e-17 against eps = 1e-8, exact zeros, moments preset for t and of mixed sign,
    m' that cancels; vector and scalar path"""
    hold = _Hold("values-t%d-betas%g-%g" % ((L["t"],) + L["betas"]))
    _hold_launch(hold, L, *_launch(dev, ext, L))
    hold.assert_ok()


def _plain(n, p, g, m, v, lr, wd, off=None):
    return dict(n=n, scale=0.0, p=p, g=g, m=m, v=v, lr=lr, wd=wd, shadow=True, off=dict(dict(p=0, g=0, m=0, v=0, s=0), **(off or {})))


def test_exact_cases(dev, ext):
    """bitwise: g = m = v = 0 leaves m' and v' at +0 and makes p' = fl(p fl(1 - lr wd)); with wd = 0 as well p' is p; lr = 0
    leaves p as it is whatever the gradient"""
    recs = []
    for n in (1024, 1027):
        p, g, m, v = R.state(n, 1.0, 3, key="exact")
        z = torch.zeros(n)
        recs += [_plain(n, p, z, z, z, 3e-3, 1e-2), _plain(n, p, z, z, z, 3e-3, 0.0), _plain(n, p, g, m, v, 0.0, 1e-2)]
    L = dict(t=3, betas=R.BETAS, eps=R.EPS, clip=None, records=recs)
    host, out, at = _launch(dev, ext, L)
    hold = _Hold("exact")
    _hold_launch(hold, L, host, out, at)
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    for i, (a, r) in enumerate(zip(at, recs)):
        got = {k: out[k][a[k]:a[k] + r["n"]] for k in "pmv"}
        if not bool(r["g"].any()):
            want = r["p"] * (f(1.0) - f(r["lr"]) * f(r["wd"]))
            hold.true(torch.equal(_bits(got["p"]), _bits(want)), "record %d: p' is not fl(p fl(1 - lr wd))" % i)
            hold.true(not bool(_bits(got["m"]).any()) and not bool(_bits(got["v"]).any()), "record %d: m' or v' is not +0" % i)
            if r["wd"] == 0:
                hold.true(torch.equal(_bits(got["p"]), _bits(r["p"])), "record %d: wd = 0, g = m = v = 0 changed p" % i)
        else:
            hold.true(torch.equal(_bits(got["p"]), _bits(r["p"])), "record %d: lr = 0 changed p" % i)
    hold.assert_ok()


def test_shadow_rounding_sweep(dev, ext):
    """lr = 0 and g = m = v = 0 keep p: every one of the 65536 low-half bit patterns under six sign / exponent / last-kept-bit
    choices -- five on the vector path, one on the scalar path (p one float off its alignment) -- must come out in the
    shadow as torch's round-to-nearest-even bf16, ties, the carry into the exponent and the overflow to infinity included"""
    vec = torch.cat([R.sweep_values(h) for h in R.SWEEP_HIGH[:5]])
    sca = R.sweep_values(R.SWEEP_HIGH[5])
    recs = [_plain(x.numel(), x, torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), 0.0, 1e-2, off)
            for x, off in ((vec, None), (sca, dict(p=1)))]
    L = dict(t=2, betas=R.BETAS, eps=R.EPS, clip=None, records=recs)
    host, out, at = _launch(dev, ext, L)
    for a, r in zip(at, recs):
        n = r["n"]
        assert torch.equal(_bits(out["p"][a["p"]:a["p"] + n]), _bits(r["p"])), "lr = 0 changed p"
        got, want = R.bf16_bits(out["s"][a["s"]:a["s"] + n]), R.bf16_bits(r["p"].to(torch.bfloat16))
        bad = (got != want).nonzero()
        assert bad.numel() == 0, "%d shadows differ, first p bits %#x: %#x, want %#x" % (
            bad.shape[0], int(_bits(r["p"])[bad[0, 0]]) & 0xFFFFFFFF, int(got[bad[0, 0]]), int(want[bad[0, 0]]))
    assert bool((out["s"].view(torch.int16)[:R.GAP] == R.CANARY16).all())


# ---- c. clamp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [1.0, None, 0.0], ids=["clip1", "clipNone", "clip0"])
def test_clamp_battery(dev, ext, clip):
    """g of +-clip, one ulp inside, one ulp outside, +-inf, NaN and -NaN in every lane of a float4 and on the scalar path:
    torch.clamp and then the reference step.  NaN in gives NaN in m', v', p' and the shadow; +-inf under clipping gives
    +-clip; without clipping (None and 0) the gradient passes untouched.  The stored gradient stays as it was, bit for bit."""
    L = R.clamp_launch(clip or None)
    host, out, at = _launch(dev, ext, L, clip=clip)
    hold = _Hold("clamp-%s" % clip)
    _hold_launch(hold, L, host, out, at)
    for a, r in zip(at, L["records"]):
        nan = torch.isnan(r["g"])
        hold.true(bool(nan.any()), "the record has no NaN gradient")
        for k in "pmv":
            hold.true(bool(torch.isnan(out[k][a[k]:a[k] + r["n"]][nan]).all()), "%s' of a NaN gradient is not NaN" % k)
        hold.true(bool(torch.isnan(out["s"][a["s"]:a["s"] + r["n"]].float()[nan]).all()), "the shadow of a NaN gradient is not NaN")
    hold.assert_ok()


# ---- d. wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_battery_three_eager_steps(dev, ext):
    """optim.FusedAdamW over 300 tiny parameters (n = 1 .. 40, a third of them views at whatever float offset a packed flat
    buffer gives them, their gradients views of a second buffer packed one float further on) and four longer ones, in three
    groups with their own lr and wd; a parameter in the middle of a group without a gradient, an empty parameter, a weight
    with a registered shadow.  Each of three steps: p, exp_avg and exp_avg_sq held to the bound from the state before it."""
    from bridgeqa_amd import fusion_ops as ops
    from bridgeqa_amd import fusion_state
    from bridgeqa_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(11)
    sizes = [1 + (7 * i) % 40 for i in range(300)] + [255, 1028, 8193, 16388]
    packed = [i for i in range(300) if i % 3 == 1]
    total = sum(sizes[i] for i in packed)
    flat_p = torch.randn(total + 3, generator=gen).to(dev)
    flat_g = torch.zeros(total + 4, device=dev)
    params, gviews, off = [], {}, 0
    for i, n in enumerate(sizes):
        if i in packed:
            params.append(torch.nn.Parameter(flat_p[off + 3:off + 3 + n]))
            gviews[i] = flat_g[off + 4:off + 4 + n]
            off += n
        else:
            params.append(torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)))
    assert any(p.data_ptr() % 16 for p in params) and any(g.data_ptr() % 16 for g in gviews.values())
    weight = torch.nn.Parameter(torch.randn(64, 64, generator=gen).to(dev))
    empty = torch.nn.Parameter(torch.empty(0, device=dev))
    idle = 150                                              # in the middle of the second group, never given a gradient
    groups = [dict(params=params[:100] + [weight], lr=3e-3, weight_decay=1e-2),
              dict(params=params[100:200] + [empty], lr=1e-2, weight_decay=0.0),
              dict(params=params[200:], lr=5e-4, weight_decay=5e-2)]
    hyper = {id(p): (g["lr"], g["weight_decay"]) for g in groups for p in g["params"]}
    everything = params + [weight, empty]
    prev = ops.set_compute_dtype(torch.bfloat16)
    hold = _Hold("wrapper")
    try:
        shadow = fusion_state._shadow(weight)
        assert ops.shadow_of(weight) is shadow and shadow.dtype == torch.bfloat16
        opt = FusedAdamW(groups, betas=R.BETAS, eps=R.EPS)
        idle_before = params[idle].detach().cpu().clone()
        for t in (1, 2, 3):
            scale = (1.0, 1e-4, 1e-8)[t - 1]
            before = []
            for i, p in enumerate(everything):
                if p is params[idle]:
                    before.append(None)
                    continue
                g = (torch.randn(p.shape, generator=gen) * scale).to(dev)
                if i in gviews:
                    gviews[i].copy_(g)
                    g = gviews[i]
                p.grad = g
                st = opt.state[p]
                zeros = torch.zeros(p.shape)
                before.append((p.detach().cpu().clone(), g.cpu().clone(), st["exp_avg"].cpu().clone() if "exp_avg" in st else zeros,
                               st["exp_avg_sq"].cpu().clone() if "exp_avg_sq" in st else zeros))
            opt.step()
            torch.cuda.synchronize()
            for i, (p, b) in enumerate(zip(everything, before)):
                if b is None:
                    continue
                lr, wd = hyper[id(p)]
                ref = R.reference(b[0].view(-1), b[1].view(-1), b[2].view(-1), b[3].view(-1), t, lr, wd, R.BETAS, R.EPS)
                what = "step %d parameter %d (n %d)" % (t, i, p.numel())
                st = opt.state[p]
                hold("p", p.detach().view(-1), ref["p"], ref["tol_p"], what)
                hold("m", st["exp_avg"].view(-1), ref["m"], ref["tol_m"], what)
                hold("v", st["exp_avg_sq"].view(-1), ref["v"], ref["tol_v"], what)
                hold.true(torch.equal(_bits(p.grad.cpu()), _bits(b[1])), what + ": the gradient changed")
            hold.true(torch.equal(R.bf16_bits(ops.shadow_of(weight)), R.bf16_bits(weight.detach().to(torch.bfloat16))),
                      "step %d: the registered shadow is not the updated weight in bf16" % t)
        hold.true(torch.equal(_bits(params[idle].detach().cpu()), _bits(idle_before)), "the parameter without a gradient changed")
        hold.true("exp_avg" not in opt.state[params[idle]] and "exp_avg_sq" not in opt.state[params[idle]],
                  "the parameter without a gradient has moments")
        hold.true(float(opt.state[params[0]]["step"]) == 3.0 and float(opt.state[weight]["step"]) == 3.0, "the counter does not read 3")
        hold.true(empty.numel() == 0 and params[idle].grad is None, "the empty / idle parameters are not what the test set up")
    finally:
        ops.set_compute_dtype(prev)
    hold.assert_ok()
