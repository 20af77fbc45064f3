"""The LDS-DMA tile loops whose LDS traffic is ordered by hand (inline-asm fragment reads and DMAs, counted vmcnt waits,
lgkmcnt(0) waits, barriers: csrc/gemm_common.h read_frag_asm / read_frag_cf_x / lds_dma16) against the same sources built with
the compiler-visible code (BQ_G256_ASM_READS=0 BQ_DMA_ASM=0 BQ_CF_ASM_READS=0: the same MFMA sequence, LDS traffic ordered by
hipcc's own waits -- tests/test_isa_waits_cpu.py holds that build to carrying them).  The two builds differ only in how LDS
traffic is ordered, so every output of the battery below must agree BIT FOR BIT; each output of the default build is also held
elementwise to an fp64 reference (a per-element bound, not a norm: one wrong 16 x 16 tile fails).

Bound, for C = A B with the absolute-value product |A| |B| and contraction length K (u = 2^-24):
    bf16 out: |out - ref64| <= 2^-8 |ref64| + C_ACC K u (|A| |B|)
    fp32 out: |out - ref64| <=              C_ACC K u (|A| |B|)
with C_ACC = 2 (recursive fp32 summation is within (K - 1) u sum |a b| of the exact sum, whatever the order; bf16 rounding of the
result is 2^-9 relative).  Epilogues are checked on their pre-activation; GELU / GELU' add the fit's error (gemm_common.h).

And the repeatability under load of the kernels that had none: 12 launches each, bit-identical to the first, while a side
stream streams through 256 MB and the L2 is evicted every third iteration (eager launches only).

    python tests/test_lds_pipeline_gpu.py OUT.pt   runs the battery in this process (the test's child)
"""
import os
import subprocess
import sys

import pytest
import torch

from load_util import _repeat_under_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FENCED_DEFINES = ("BQ_G256_ASM_READS=0", "BQ_DMA_ASM=0", "BQ_CF_ASM_READS=0")
FENCED_SOURCES = ("gemm.hip", "gemm_mid.hip", "detbwd.hip")
C_ACC = 2.0
U = 2.0 ** -24

# the 10 shapes of tests/test_modules_gpu.py::test_fused_sharedmlp_backward: R, K, ldx, N, S, pool, need_dx
SA_SHAPES = [(131072, 64, 64, 64, 64, False, True), (131072, 64, 64, 128, 64, True, True), (70001, 135, 136, 64, 64, False, False),
             (70016, 131, 136, 128, 32, False, True), (98304, 128, 128, 128, 32, False, True), (65536, 128, 128, 128, 16, True, True),
             (131072, 64, 64, 64, 32, True, False), (65536, 128, 128, 256, 32, True, True), (65600, 128, 128, 256, 16, True, True),
             (69632, 131, 136, 128, 16, True, True)]
# the 13 shapes of tests/test_gemm_gpu.py::test_wgrad_rows: R, N, K
WGRAD_SHAPES = [(70001, 64, 136), (33000, 128, 64), (9000, 256, 120), (5000, 64, 64), (4100, 128, 136), (3000, 128, 128),
                (2500, 256, 64), (2000, 64, 248), (1500, 128, 200), (64, 64, 72), (130, 128, 192), (5000, 128, 264),
                (3000, 256, 136)]


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(torch.bfloat16)


def _mm64(a, b):
    """(a b, |a| |b|) in fp64"""
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def _gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5))


def _dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5


class _Checker:
    """collects the elementwise violations of the bound above (the battery runs on, the test reports all of them)"""

    def __init__(self):
        self.failures, self.checked = [], 0

    def __call__(self, name, out, ref, absprod, K, bf16, extra=None):
        err = (out.double() - ref).abs()
        tol = C_ACC * K * U * absprod + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
        if extra is not None:
            tol = tol + extra
        bad = ~(err <= tol)
        self.checked += out.numel()
        if bad.any():
            idx = tuple(int(v) for v in bad.nonzero()[0])
            self.failures.append("%s: %d of %d elements out of bound, first at %s: out %r ref %r tol %r" % (
                name, int(bad.sum()), out.numel(), idx, float(out[idx]), float(ref[idx]), float(tol[idx])))


def _gemm_family(dev, res, chk, tile):
    """the forms of one tile class: forward (none, bias, bias + GELU), dX (none, add, dGELU [+ colsum]), dW, grouped ragged"""
    from bridgeqa_amd import _ext
    t = "t%d" % tile
    # forward: one K tile (prologue only), two and three K tiles, M not a multiple of 256, N not a multiple of 128, c3 fc2
    fwd = [(1000, 512, 64), (257, 264, 128), (1000, 392, 192), (2100, 1024, 256)]
    if tile >= 128:
        fwd += [(16400, 768, 3072)]
    for s, (M, N, K) in enumerate(fwd):
        if tile == 128 and K < 128:
            continue   # (the 256 x 128 kernel's DMA stream runs two K tiles ahead: K >= 128)
        x, w = _rand((M, K), dev, 100 + s), _rand((N, K), dev, 120 + s, 0.1)
        b = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(140 + s))
        ref, ab = _mm64(x, w.t())
        key = "%s/fwd/%dx%dx%d" % (t, M, N, K)
        res[key + "/none"] = y0 = _ext.gemm_fwd(x, w, None, tile=tile)
        chk(key + "/none", y0, ref, ab, K, True)
        res[key + "/bias"] = yb = _ext.gemm_fwd(x, w, b, tile=tile)
        chk(key + "/bias", yb, ref + b.double(), ab + b.double().abs(), K + 1, True)
        if M * N <= 4e6 or tile >= 128:
            y, act = _ext.gemm_fwd(x, w, b, gelu=True, tile=tile)
            res[key + "/gelu.pre"], res[key + "/gelu.act"] = y, act
            chk(key + "/gelu.pre", y, ref + b.double(), ab + b.double().abs(), K + 1, True)
            # the activation is taken at the stored pre-activation; the fit is within 3.1e-5 of gelu_erf
            g = _gelu64(y.double())
            chk(key + "/gelu.act", act, g, torch.zeros_like(g), 1, True, extra=4e-5)
        del ref, ab
    # dX = dY W: contraction over N (P contraction-major: transposed LDS reads), c3 fc2's dX
    dxs = [(1000, 64, 512), (1000, 384, 512), (1500, 192, 264), (320, 768, 3072)]
    if tile >= 128:
        dxs += [(16400, 3072, 768)]
    for s, (M, N, K) in enumerate(dxs):
        if tile == 128 and N < 128:
            continue
        dy, w = _rand((M, N), dev, 200 + s), _rand((N, K), dev, 220 + s, 0.1)
        pre, other = _rand((M, K), dev, 240 + s, 1.5), _rand((M, K), dev, 260 + s)
        ref, ab = _mm64(dy, w)
        key = "%s/dx/%dx%dx%d" % (t, M, N, K)
        res[key + "/none"] = d0 = _ext.gemm_dx(dy, w, tile=tile)
        chk(key + "/none", d0, ref, ab, N, True)
        res[key + "/add"] = da = _ext.gemm_dx(dy, w, add=other, tile=tile)
        chk(key + "/add", da, ref + other.double(), ab + other.double().abs(), N + 1, True)
        cs = torch.zeros(K, device=dev) if tile != 128 else None
        res[key + "/dgelu"] = dg = _ext.gemm_dx(dy, w, pre_act=pre, colsum=cs, tile=tile)
        gp = _dgelu64(pre.double())
        chk(key + "/dgelu", dg, ref * gp, ab * gp.abs(), N, True, extra=1.3e-4 * ref.abs())
        if cs is not None:   # (fp32 atomics across row tiles: in the fp64 check, not in the bit comparison)
            # (the column sums may be taken before the bf16 rounding of dX: 2^-8 of sum |dX| on top)
            s_abs = dg.double().abs().sum(0)
            chk(key + "/dgelu.colsum", cs, dg.double().sum(0), s_abs, M, False, extra=2.0 ** -8 * s_abs)
        if tile == 128:   # dX on a transposed weight (wt=): K-contiguous like a forward
            res[key + "/wt"] = dt = _ext.gemm_dx(dy, w, wt=w.t().contiguous(), tile=tile)
            chk(key + "/wt", dt, ref, ab, N, True)
        del ref, ab
    # dW = dY^T X in fp32: both operands contraction-major; contractions of 1 .. 3 K tiles, ragged ones, the short weight
    # gradients of 80 and 20 rows
    if tile != 32:
        dws = [(64, 256, 256), (128, 512, 256), (192, 256, 768), (1000, 512, 768), (80, 768, 768), (20, 768, 1536),
               (1025, 776, 320)]
        for s, (M, N, K) in enumerate(dws):
            if tile == 128 and M < 128:
                continue   # (the persistent 256 x 128 kernel needs two K tiles)
            dy, x = _rand((M, N), dev, 300 + s), _rand((M, K), dev, 320 + s)
            ref, ab = _mm64(dy.t(), x)
            key = "%s/dw/%dx%dx%d" % (t, M, N, K)
            res[key] = dw = _ext.gemm_dw(dy, x, tile=tile)
            chk(key, dw, ref, ab, M, False)
    # one grouped launch of ragged problems (Ni not a multiple of 256, Nj not of 128)
    if tile >= 128:
        probs, refs = [], []
        for k, (M, N, K) in enumerate([(1000, 264, 192), (129, 768, 768), (70, 8, 128), (4416, 1536, 768)]):
            x, w = _rand((M, K), dev, 400 + k), _rand((N, K), dev, 420 + k, 0.1)
            b = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(440 + k))
            probs.append(dict(P=w, Q=x, out=torch.empty(M, N, device=dev, dtype=torch.bfloat16), bias=b))
            refs.append((_mm64(x, w.t()), b, K))
        _ext.gemm_grouped(probs, 0, _ext.EPI_BIAS, tile)
        for k, (p, ((r, ab), b, K)) in enumerate(zip(probs, refs)):
            res["%s/grouped/%d" % (t, k)] = p["out"]
            chk("%s/grouped/%d" % (t, k), p["out"], r + b.double(), ab + b.double().abs(), K + 1, True)
    if tile == 128:
        # the stream-K form of the 256 x 128 kernel (tiles cut across workgroups, finished through the workspace): taken only
        # when whole tiles fill the grid unevenly and a share is >= 16 K tiles (launch_gemm_mid) -- the c3 fc2 forward is such
        # a launch.  Its fp32 summation order differs from the whole-tile launch of the same inputs: equal results would mean
        # the stream-K path was not taken.
        M, N, K = 16400, 768, 3072
        x, w = _rand((M, K), dev, 500), _rand((N, K), dev, 501, 0.05)
        ref, ab = _mm64(x, w.t())
        key = "t128/streamk/%dx%dx%d" % (M, N, K)
        prev = _ext.STREAMK[0]
        try:
            _ext.streamk_enable(False)
            res[key + "/whole"] = yw = _ext.gemm_fwd(x, w, None, tile=128)
            _ext.streamk_enable(True)
            res[key] = ys = _ext.gemm_fwd(x, w, None, tile=128)
        finally:
            _ext.streamk_enable(prev)
        chk(key + "/whole", yw, ref, ab, K, True)
        chk(key, ys, ref, ab, K, True)
        if torch.equal(ys, yw):
            chk.failures.append("%s: bitwise equal to the whole-tile launch -- the stream-K path was not taken" % key)
        del ref, ab


def _wgrad_rows(dev, res, chk):
    from bridgeqa_amd import _ext
    for s, (R, N, K) in enumerate(WGRAD_SHAPES):
        dy = _rand((R, N), dev, 600 + s)
        ld = K + 8
        xbuf = torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)
        xbuf[:, :K] = _rand((R, K), dev, 620 + s)
        ref, ab = _mm64(dy.t(), xbuf)
        for wgs in (0, 7):
            key = "wgrad_rows/%dx%dx%d/wgs%d" % (R, N, K, wgs)
            res[key + "/rows"] = o1 = _ext.wgrad_rows(torch.as_strided(xbuf, (R, ld), (ld, 1)), dy,
                                                      torch.full((N, ld), float("nan"), device=dev), wgs)
            chk(key + "/rows", o1, ref, ab, R, False)
            res[key + "/cols"] = o2 = _ext.wgrad_rows(xbuf[:, :K], dy, torch.full((N, K), float("nan"), device=dev), wgs)
            chk(key + "/cols", o2, ref[:, :K], ab[:, :K], R, False)


def _sa_inputs(dev, R, K, ldx, N, S, pool):
    g = torch.Generator().manual_seed(R % 977 + N + S)
    xfull = torch.zeros(R, ldx)
    xfull[:, :K] = torch.randn(R, K, generator=g)
    w = torch.zeros(N, (ldx + 63) // 64 * 64)
    w[:, :K] = torch.randn(N, K, generator=g) / K ** 0.5
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    dout = torch.randn(R // S if pool else R, N, generator=g)
    xs = torch.zeros(4, ldx)
    xs[0, :K], xs[1, :K], xs[3] = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3, 1.0
    return (xfull.to(dev).to(torch.bfloat16), w.to(dev).to(torch.bfloat16), gamma.to(dev), beta.to(dev),
            dout.to(dev).to(torch.bfloat16), xs.to(dev))


def _sa_forward(x, K, w, gamma, beta, S, pool, x_stats=None):
    from bridgeqa_amd import _ext
    N = w.shape[0]
    rm, rv = torch.zeros(N, device=x.device), torch.ones(N, device=x.device)
    nbt = torch.zeros((), dtype=torch.long, device=x.device)
    rows = x[:, :K] if x.shape[1] != K else x
    r = _ext.pwconv_bn_relu_fwd(rows, K, w, gamma, beta, rm, rv, nbt, 1e-5, 0.1, S, True, pool, want_arg=pool,
                                x_stats=x_stats)
    return r if pool else tuple(r) + (None,)


def _layer_input(x, K, x_stats):
    """the layer's input rows in fp64: x itself, or relu(x xscale + xshift) (fp32 arithmetic, as the kernels; not rounded to
    bf16 -- the kernels' rounding of it is in the bound)"""
    if x_stats is None:
        return x[:, :K].double()
    return torch.relu(x[:, :K].float() * x_stats[0, :K] + x_stats[1, :K]).double()


def _sa_dp64(y_raw, dout, arg, stats, dgb, S, pool):
    """dP of csrc/detbwd.hip in fp64 and |its three terms| (the fp32 evaluation and bf16 rounding of dP are in the bound):
    dP = sc g + c0 + y c1, c1 = -sc rstd dgamma / R, c0 = -sc dbeta / R - c1 mean; g = dOut (routed to the arg-max row of its
    group when pooled) masked where y sc + sh <= 0 (evaluated in fp32, as the kernel)"""
    R = y_raw.shape[0]
    sc, sh, mean, rstd = (stats[i].double() for i in range(4))
    g = dout.double()
    if pool:
        rows = torch.arange(R, device=y_raw.device) % S
        g = g.repeat_interleave(S, 0) * (arg.long().repeat_interleave(S, 0) == rows[:, None])
    g = g * ((y_raw.float() * stats[0] + stats[1]) > 0)
    c1 = -sc * rstd * dgb[1].double() / R
    c0 = -sc * dgb[0].double() / R - c1 * mean
    y = y_raw.double()
    return sc * g + c0 + y * c1, (sc * g).abs() + c0.abs() + (y * c1).abs()


def _sharedmlp(dev, res, chk):
    """pwconv_bn_relu_fwd (pwconv64s) and sa_bwd_fused (sa_bwd, with and without x_stats) on the 10 shapes.  The fp64 check
    covers their two plain products, y_raw = X W^T and dW = dP^T X, with 2^-7 of the absolute-value product on top for the bf16
    rounding of the operands formed in the kernels (dP; relu(x xscale + xshift)); the rest is held to the unfused path and
    fp32 autograd by tests/test_modules_gpu.py::test_fused_sharedmlp_backward"""
    from bridgeqa_amd import _ext
    for (R, K, ldx, N, S, pool, need_dx) in SA_SHAPES:
        x, w, gamma, beta, dout, xs = _sa_inputs(dev, R, K, ldx, N, S, pool)
        assert _ext.sa_bwd_supported(ldx, N, S, pool, need_dx)
        variants = [None] + ([xs] if need_dx and ldx == K else [])
        for x_stats in variants:
            key = "sa/%dx%dx%dx%d/S%d%s%s%s" % (R, K, ldx, N, S, "/pool" if pool else "", "/dx" if need_dx else "",
                                                "/x_stats" if x_stats is not None else "")
            out, y_raw, stats, arg = _sa_forward(x, K, w, gamma, beta, S, pool, x_stats)
            res[key + "/fwd.out"], res[key + "/fwd.y_raw"], res[key + "/fwd.stats"] = out, y_raw, stats
            if arg is not None:
                res[key + "/fwd.arg"] = arg
            dgb = _ext.bn_bwd_reduce(dout, y_raw, stats, S, True, pool, arg)
            r = _ext.sa_bwd_fused(x, y_raw, dout, arg, w, stats, dgb, S, True, pool, need_dx, x_stats=x_stats)
            res[key + "/bwd.dgb"], res[key + "/bwd.dw"] = dgb, r[1]
            if need_dx:
                res[key + "/bwd.dx"] = r[0]
            xin = _layer_input(x, K, x_stats)
            wk = w[:, :K].double()
            extra = x_stats is not None
            ref, ab = xin @ wk.t(), xin.abs() @ wk.abs().t()
            chk(key + "/fwd.y_raw", y_raw, ref, ab, K, True, extra=2.0 ** -7 * ab if extra else None)
            dp, dpa = _sa_dp64(y_raw, dout, arg, stats, dgb, S, pool)
            ref, ab = dp.t() @ xin, dpa.t() @ xin.abs()
            chk(key + "/bwd.dw", r[1][:, :K], ref, ab, R, False, extra=2.0 ** -7 * ab)
            del xin, ref, ab, dp, dpa


def battery(dev, chk=None):
    """{name: output tensor} of every template instance with a rewritten LDS loop, all inputs from fixed seeds"""
    chk = chk or _Checker()
    res = {}
    with torch.no_grad():
        for tile in (256, 128, 64, 32):
            _gemm_family(dev, res, chk, tile)
        _wgrad_rows(dev, res, chk)
        _sharedmlp(dev, res, chk)
    torch.cuda.synchronize()
    return res


# ---- the fenced library: built once per session into a temporary directory ----------------------------------------------
@pytest.fixture(scope="module")
def fenced_lib(tmp_path_factory):
    import time
    from bridgeqa_amd import build as hip_build
    objdir = os.path.join(hip_build.PKG, "build")
    others = [os.path.join(objdir, os.path.basename(s) + ".o") for s in hip_build.sources()
              if os.path.basename(s) not in FENCED_SOURCES]
    missing = [o for o in others if not os.path.exists(o)]
    assert not missing, "the default build's objects are missing (run build() first): %s" % missing
    td = str(tmp_path_factory.mktemp("fenced"))
    t0 = time.time()
    procs = []
    for src in FENCED_SOURCES:   # (3 compiles in parallel, each under its own time limit)
        obj = os.path.join(td, src + ".o")
        cmd = ["timeout", "-k", "10", "900", hip_build.HIPCC] + hip_build.FLAGS + ["-D" + d for d in FENCED_DEFINES] + \
              ["-c", os.path.join(hip_build.CSRC, src), "-o", obj]
        procs.append((src, obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    objs = []
    for src, obj, p in procs:
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, "fenced compile of %s failed (%d):\n%s" % (src, p.returncode, log[-4000:])
        objs.append(obj)
    lib = os.path.join(td, "libbqhip_fenced.so")
    subprocess.run(["timeout", "-k", "10", "300", hip_build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib]
                   + objs + others, check=True)
    # (as build(): a kernel whose body fails the host pass loses its launch stub without a diagnostic)
    syms = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    lost = [l.split()[-1] for l in syms.splitlines() if "__device_stub__" in l]
    assert not lost, "fenced build: kernels without a host launch stub: %s" % ", ".join(lost)
    sys.stdout.write("\nfenced library built in %.1f s\n" % (time.time() - t0))
    return lib


def _run_child(out, lib=None):
    env = dict(os.environ)
    env.pop("BQHIP_LIB", None)
    if lib:
        env["BQHIP_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = p.stdout.decode(errors="replace")
    assert p.returncode == 0, "battery child (%s) exited with %d:\n%s" % (lib or "default build", p.returncode, log[-6000:])
    return torch.load(out)


def test_default_build_equals_the_compiler_fenced_build_bit_for_bit(fenced_lib, tmp_path):
    # one child at a time: at most this process and one child have the GPU open
    a = _run_child(str(tmp_path / "default.pt"))
    b = _run_child(str(tmp_path / "fenced.pt"), fenced_lib)
    assert a["lib"] != b["lib"] and b["lib"] == fenced_lib
    assert not a["failures"], "default build outside the fp64 bound:\n" + "\n".join(a["failures"][:20])
    ra, rb = a["out"], b["out"]
    assert set(ra) == set(rb)
    elements = 0
    for name in sorted(ra):
        x, y = ra[name], rb[name]
        elements += x.numel()
        if not torch.equal(x, y):
            d = (x != y) if x.dtype in (torch.uint8, torch.int64) else ~((x == y) | (torch.isnan(x) & torch.isnan(y)))
            if not d.any():
                continue
            idx = tuple(int(v) for v in d.nonzero()[0])
            pytest.fail("%s differs between the default and the fenced build: %d of %d elements, first at %s: %r vs %r"
                        % (name, int(d.sum()), x.numel(), idx, x[idx].item(), y[idx].item()))
    sys.stdout.write("\n%d outputs, %d elements bit-identical; %d elements within the fp64 bound\n"
                     % (len(ra), elements, a["checked"]))


# ---- repeatability under load ---------------------------------------------------------------------------------------------
def test_contraction_major_gemm_repeatable_under_load(dev):
    from bridgeqa_amd import _ext
    dy, x = _rand((16400, 768), dev, 700), _rand((16400, 768), dev, 701)
    dy2, x2 = _rand((1000, 512), dev, 702), _rand((1000, 768), dev, 703)
    dy3, w3 = _rand((2000, 768), dev, 704), _rand((768, 3072), dev, 705, 0.05)
    _repeat_under_load(dev, [
        lambda: (_ext.gemm_dw(dy2, x2, tile=64),),          # gemm64: contraction-major dW
        lambda: (_ext.gemm_dw(dy, x, tile=128),),           # gemm128 with Q_XC
        lambda: (_ext.gemm_dx(dy3, w3, tile=64),),          # gemm64: contraction-major P
    ])


def test_wgrad_rows_repeatable_under_load(dev):
    from bridgeqa_amd import _ext
    fns = []
    for s, (R, N, K) in enumerate([(70001, 64, 136), (9000, 256, 120), (3000, 256, 136)]):
        dy, x = _rand((R, N), dev, 710 + s), _rand((R, K), dev, 720 + s)
        for wgs in (0, 7):
            fns.append(lambda dy=dy, x=x, N=N, K=K, wgs=wgs: (_ext.wgrad_rows(x, dy, torch.empty(N, K, device=dev), wgs),))
    _repeat_under_load(dev, fns)


def test_pwconv_and_sa_bwd_repeatable_under_load(dev):
    from bridgeqa_amd import _ext
    fns = []
    for (R, K, ldx, N, S, pool, need_dx) in [SA_SHAPES[3], SA_SHAPES[5], SA_SHAPES[7]]:
        x, w, gamma, beta, dout, xs = _sa_inputs(dev, R, K, ldx, N, S, pool)
        out, y_raw, stats, arg = _sa_forward(x, K, w, gamma, beta, S, pool)
        dgb = _ext.bn_bwd_reduce(dout, y_raw, stats, S, True, pool, arg)
        fns.append(lambda x=x, K=K, w=w, gamma=gamma, beta=beta, S=S, pool=pool:
                   tuple(t for t in _sa_forward(x, K, w, gamma, beta, S, pool) if t is not None))
        fns.append(lambda x=x, y_raw=y_raw, dout=dout, arg=arg, w=w, stats=stats, dgb=dgb, S=S, pool=pool, need_dx=need_dx:
                   tuple(t for t in _ext.sa_bwd_fused(x, y_raw, dout, arg, w, stats, dgb, S, True, pool, need_dx)[:2]
                         if t is not None))
    _repeat_under_load(dev, fns)


if __name__ == "__main__":
    from bridgeqa_amd import _ext
    chk = _Checker()
    out = battery(torch.device("cuda:0"), chk)
    torch.save(dict(out={k: v.detach().cpu() for k, v in out.items()}, failures=chk.failures, checked=chk.checked,
                    lib=_ext._LIB_PATH), sys.argv[1])
    print("battery: %d outputs, %d failures" % (len(out), len(chk.failures)))
