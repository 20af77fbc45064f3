"""Reference, bound, emulation, planted defects and input batteries of the fused multi-tensor AdamW step (adamw_kernel,
csrc/adamw.hip), for tests/test_adamw_bound_cpu.py and tests/test_adamw_bound_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  One step in fp64 from a given fp32 state (p, g, m, v) at the 1-based step count t -- torch's single-tensor AdamW
(amsgrad = False, maximize = False) behind clip_grad_value_:
    g <- clamp(g, -clip, clip)  (torch.clamp: NaN stays NaN; no clipping: g as it is)
    q = p (1 - lr wd)           m' = b1 m + (1 - b1) g          v' = b2 v + (1 - b2) g g
    upd = (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)           p' = q - upd
lr, wd, b1, b2, eps and clip are the fp32-ROUNDED values the kernel receives (the launcher passes C floats, the table holds f32
lr and wd): with them the kernel is self-consistent (1 - b2 and 1 - b2^t carry the same rounding of b2); double 0.999 would
charge it 1.3e-5 that is not its error.  b1, b2 >= 0.5, so that 1 - b is exact in fp32 (asserted).

BOUND.  u = 2^-24; every fp32 operation of the kernel (the build has -O3 -ffp-contract=off and no fast-math, so * + - / and
sqrtf are one correct rounding each) is counted in the kernel's expression order, each rounding at its worst case u |result|.
That count is attained by correct arithmetic to within a quarter (the emulation below reaches 0.74 of it on p' and 0.61 on
m'), so every ROUNDING term of the tolerance is taken H = 2 times: a correct kernel then stays within half of the bound and
every planted defect is still orders of magnitude outside it.  The powf term is not doubled.  S = |b1 m| + |(1 - b1) g|.
  m'   H 3 u (1 + u) S          two products and one sum, each rounding at most u (1 + u) S.  S, not |m'|: the two terms cancel.
  v'   H 4 u (1 + 2 u) v'       b2 v: one rounding; ((1 - b2) g) g: two; the sum: one; every term is non-negative.
  p'   (1 + 2^-10) { H [ u (2 |q| + |p| lr wd) + u (|q| + |upd|) + 3 u updS + |upd| (4 u + rden) ] + |upd| (pow1 + pow2 A / (2 D)) }
       q: lr wd, 1 - lr wd and p decay round once each; the last subtraction rounds once (|p'| <= |q| + |upd|);
       updS = (lr / (1 - b1^t)) S / D is the update of the MAGNITUDES (the absolute error of m', carried through);
       4 u: 1 - powf(b1, t) (exact while b1^t >= 0.5), the step size lr / bc1, m' / denom and the product with the step size;
       rden = 6.5 u A / D + u,   A = sqrt(v') / sqrt(1 - b2^t),  D = A + eps: v' (4 u, halved by the root), sqrtf (u),
               1 / sqrtf(bc2) (u / 2 for the subtraction in bc2, 2 u), their product (u), weighted by A's share of the
               denominator; the sum with eps (u);
       pow_i = K_POW u b_i^t / (1 - b_i^t): the error of powf amplified by the cancellation in the fp32 bias correction
               1 - powf(b_i, t); the root halves it for b2, and A / D is again the share of the denominator it acts on.
       The factor 1 + 2^-10 covers the products of these first-order terms (the largest, K_POW u 999 at t = 1, is 1.2e-4).
  The cancellation in 1 - powf(b, t) is real and large early (b2 = 0.999: about 250 u possible at t = 2, under 0.2 u from
  t = 1000), inherent to fp32 bias corrections (torch's capturable path has it too), and so part of the bound.
  K_POW = 2: no document available to this suite states the accuracy of the device powf, so the bound allows it
  2 u b^t -- one ulp of the result wherever it lies in its binade, twice the error of a correctly rounded powf (the emulation's).
  Where the reference is NaN the output must be NaN; where it is +-inf the output must be that infinity.

INPUTS.  Every battery keeps every intermediate zero or a NORMAL fp32 number (emulate() returns them; the CPU suite asserts
it): the smallest gradients are 4e-18, where (1 - b2) g^2 = 1.6e-38 is still normal; nothing wanders into subnormals, whose
absolute rounding error the relative bound does not model.

The emulation restates the per-element lines of adamw_kernel (csrc/adamw.hip) in fp32 torch on the CPU, in their order, powf correctly rounded, with the planted defects
of the CPU suite as switches.
"""
import functools
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
K_POW = 2.0
H = 2.0                     # headroom on the rounding terms (module docstring)
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -126          # the smallest normal fp32 number
CHUNK = 8192                # elements per workgroup (bq_adamw_chunk_elems(); the GPU suite asserts it)
RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("s", "<u8"), ("n", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
CANARY32 = -889275714       # 0xCAFEBABE as int32: the bits of the gaps between the tensors of an fp32 arena
CANARY16 = -16657           # 0xBEEF as int16: the same in the bf16 shadow arena
GAP = 8                     # canary elements (at least) before and after every tensor


def f32(x):
    """the C float nearest to the Python float x, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def _clipv(clip):
    return f32(clip) if clip else math.inf


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


# ---- reference and bound --------------------------------------------------------------------------------------------------------
def reference(p, g, m, v, t, lr, wd, betas=(0.9, 0.999), eps=1e-8, clip=None):
    """dict of fp64 tensors: p, m, v (the new state), q and upd (the two parts of p), root (the bias-corrected sqrt(v') that
    meets eps in the denominator), tol_p, tol_m, tol_v"""
    lr, wd, b1, b2, eps = f32(lr), f32(wd), f32(betas[0]), f32(betas[1]), f32(eps)
    assert 0.5 <= b1 < 1.0 and 0.5 <= b2 < 1.0 and t >= 1
    c = _clipv(clip)
    P, G, M, V = p.double(), g.double(), m.double(), v.double()
    gc = torch.clamp(G, -c, c)
    q = P * (1.0 - lr * wd)
    a, b = b1 * M, (1.0 - b1) * gc
    m1 = a + b
    v1 = b2 * V + (1.0 - b2) * gc * gc
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    A = torch.sqrt(v1) / math.sqrt(bc2)
    D = A + eps
    upd = (lr / bc1) * m1 / D
    p1 = q - upd
    S = a.abs() + b.abs()
    pow1, pow2 = K_POW * U * pw1 / bc1, K_POW * U * pw2 / bc2
    share = A / D
    rden = 6.5 * U * share + U
    updS = (lr / bc1) * S / D
    rounding = (U * (2.0 * q.abs() + P.abs() * lr * wd) + U * (q.abs() + upd.abs()) + 3.0 * U * updS + upd.abs() * (4.0 * U + rden))
    tol_p = SLACK * (H * rounding + upd.abs() * (pow1 + pow2 * share / 2.0))
    return dict(p=p1, m=m1, v=v1, q=q, upd=upd, root=A, tol_p=tol_p, tol_m=H * 3.0 * U * (1.0 + U) * S, tol_v=H * 4.0 * U * (1.0 + 2.0 * U) * v1)


def excess(out, ref, tol):
    """(worst |err| / tol over the finite elements with tol > 0, message or None).  `not (err <= tol)` fails, so NaN fails, and
    where tol is 0 anything but the reference's value fails.  Where the reference is NaN the output must be NaN (isnan on
    both), where it is +-inf the output must equal it.  The message gives the count, the worst ratio and the first offender."""
    out = out.detach().cpu().double().reshape(ref.shape)
    rnan, rinf = torch.isnan(ref), torch.isinf(ref)
    fin = ~(rnan | rinf)
    zero = torch.zeros_like(ref)
    err = torch.where(fin, (out - ref).abs(), zero)
    bad = torch.where(rnan, ~torch.isnan(out), torch.where(rinf, out != ref, ~(err <= tol)))
    held = fin & (tol > 0)
    ratio = float((err[held] / tol[held]).max()) if held.any() else 0.0
    if not bad.any():
        return ratio, None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return float("inf") if ratio != ratio else ratio, "%d of %d out of bound (|err| / tol up to %.3g), first at %s: out %r ref %r tol %.3e" % (
        int(bad.sum()), out.numel(), ratio, idx, float(out[idx]), float(ref[idx]), float(tol[idx]))


def old_allclose_accepts(p_out, p_ref):
    """the comparison of tests/test_attn_gpu.py::test_fused_adamw_matches_torch_adamw_and_writes_the_shadows, on p alone"""
    return bool(torch.allclose(p_out.float(), p_ref.float(), rtol=2e-6, atol=2e-7))


def bf16_bits(s):
    """the 16-bit patterns of a bf16 tensor, as int64"""
    return s.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bf16_bits_rne(x):
    """the bit patterns of the round-to-nearest-even bf16 of a finite fp32 tensor, by integer arithmetic: what torch's cast
    is checked against before the GPU suite uses it as the reference of the shadows"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (b + 0x7FFF + ((b >> 16) & 1)) >> 16


# ---- fp32 emulation of the kernel's arithmetic ----------------------------------------------------------------------------------
DEFECTS = ("no_eps", "eps_under_root", "eps_scaled", "bc_from_t_minus_1", "bc2_without_root", "wd_after_update", "wd_of_neighbour",
           "m_from_unclamped_g", "v_from_g", "clamp_of_abs", "nan_to_minus_clip", "shadow_truncated", "tail_skipped",
           "last_chunk_skipped")


def emulate(p, g, m, v, t, lr, wd, betas=(0.9, 0.999), eps=1e-8, clip=None, defect=None, wd_neighbour=None):
    """dict p, m, v (fp32), shadow (bf16) and mids (every intermediate, for the normal-number check) of one step with the
    kernel's rounding points.  defect: one of DEFECTS or None; wd_neighbour: the next record's wd (for "wd_of_neighbour")."""
    assert defect is None or defect in DEFECTS
    T = lambda x: torch.tensor(x, dtype=torch.float32)
    one = T(1.0)
    if defect == "wd_of_neighbour":
        wd = wd_neighbour
    lr_, wd_, b1, b2, eps_ = T(lr), T(wd), T(betas[0]), T(betas[1]), T(eps)
    c = T(_clipv(clip))
    tt = t - 1 if defect == "bc_from_t_minus_1" else t
    bc1, bc2 = one - T(float(b1) ** tt), one - T(float(b2) ** tt)      # powf correctly rounded
    step_size = lr_ / bc1
    inv_sqrt_bc2 = one / (bc2 if defect == "bc2_without_root" else torch.sqrt(bc2))
    decay = one - lr_ * wd_
    omb1, omb2 = one - b1, one - b2
    gj = torch.clamp(g, -c, c)
    if defect == "clamp_of_abs":
        gj = torch.clamp(g.abs(), -c, c)
    if defect == "nan_to_minus_clip":                                  # fminf(fmaxf(g, -clip), clip): fmaxf drops the NaN
        gj = torch.where(torch.isnan(g), -c, gj)
    gm = g if defect == "m_from_unclamped_g" else gj
    q = p * decay
    t1, t2 = b1 * m, omb1 * gm
    m1 = t1 + t2
    t3, t4 = b2 * v, omb2 * gj
    t5 = t4 if defect == "v_from_g" else t4 * gj
    v1 = t3 + t5
    r = torch.sqrt(v1 + eps_) if defect == "eps_under_root" else torch.sqrt(v1)
    if defect == "eps_scaled":
        denom = (r + eps_) * inv_sqrt_bc2
    else:
        sc = r * inv_sqrt_bc2
        denom = sc if defect in ("no_eps", "eps_under_root") else sc + eps_
    quo = m1 / denom
    ups = step_size * quo
    p1 = (p - ups) * decay if defect == "wd_after_update" else q - ups
    n = p.numel()
    skip = n - n % 4 if defect == "tail_skipped" else (n - 1) // CHUNK * CHUNK if defect == "last_chunk_skipped" else n
    if skip < n:
        p1, m1, v1 = (torch.cat([new[:skip], old[skip:]]) for new, old in ((p1, p), (m1, m), (v1, v)))
    if defect == "shadow_truncated":
        shadow = (p1.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    else:
        shadow = p1.to(torch.bfloat16)
    return dict(p=p1, m=m1, v=v1, shadow=shadow, mids=[q, t1, t2, m1, t3, t4, t5, v1, r, denom, quo, ups, p1])


def all_zero_or_normal(ts):
    return all(bool(((x == 0) | ((x.abs() >= TINY) & torch.isfinite(x))).all()) for x in ts)


# ---- batteries: seeded, shared between the CPU and the GPU suite; do not write to the tensors ----------------------------------
SCALES = (1.0, 1e-4, 1e-8, 1e-12, 1e-17)      # gradient magnitudes scale x [0.4, 2.5]: the last reaches down to 4e-18
STEPS = (1, 2, 3, 10, 1000, 100000)
BETAS = (0.9, 0.999)
OTHER_BETAS = (0.5, 0.9)
EPS = 1e-8
LR_WD = ((3e-3, 1e-2), (1e-2, 0.0), (0.0, 5e-2))


def _mag(gen, n):
    return torch.exp((torch.rand(n, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * math.log(2.5))


def _sign(gen, n):
    return torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0


def state(n, scale, t, betas=BETAS, key=()):
    """fp32 p, g, m, v of n elements.  |p| in 0.01 + |N(0, 1)|; g = +-scale x [0.4, 2.5], every 7th element (from 0) exactly 0;
    t = 1: fresh moments (0); t > 1: moments consistent with t steps of such gradients, m = +-0.3 (1 - b1^t) scale x [0.4, 2.5]
    and v = (1 - b2^t) (scale x [0.4, 2.5])^2 (so that the bias-corrected root stays at the gradient's scale at every t),
    except that every 5th element (from 1) has m = -(1 - b1) g / b1, so that m' cancels to a few ulp of its terms or to 0, and
    every 11th (from 3) has g = m = v = 0."""
    gen = torch.Generator().manual_seed(_seed("adamw", n, scale, t, betas, key))
    i = torch.arange(n)
    p = (_sign(gen, n) * (0.01 + torch.randn(n, generator=gen, dtype=torch.float64).abs())).float()
    g = (_sign(gen, n) * scale * _mag(gen, n)).float()
    g[i % 7 == 0] = 0.0
    m, v = torch.zeros(n), torch.zeros(n)
    if t > 1:
        m = (_sign(gen, n) * 0.3 * (1.0 - betas[0] ** t) * scale * _mag(gen, n)).float()
        v = ((1.0 - betas[1] ** t) * (scale * _mag(gen, n)) ** 2).float()
        b1 = torch.tensor(betas[0], dtype=torch.float32)
        m = torch.where(i % 5 == 1, -((1.0 - b1) * g) / b1, m)
        dead = i % 11 == 3
        g[dead], m[dead], v[dead] = 0.0, 0.0, 0.0
    return p, g, m, v


def record(n, scale, t, betas=BETAS, lr=LR_WD[0][0], wd=LR_WD[0][1], shadow=True, off=None, key=()):
    p, g, m, v = state(n, scale, t, betas, key)
    return dict(n=n, scale=scale, p=p, g=g, m=m, v=v, lr=lr, wd=wd, shadow=shadow, off=dict(dict(p=0, g=0, m=0, v=0, s=0), **(off or {})))


@functools.lru_cache(maxsize=None)
def value_launch(t, betas=BETAS):
    """one launch of the value battery: per gradient scale a vector-path record (n = 1024) and a scalar-path one (n = 1027)"""
    recs = [record(n, s, t, betas, key="value") for s in SCALES for n in (1024, 1027)]
    return dict(t=t, betas=betas, eps=EPS, clip=None, records=recs)


def value_launches():
    return [value_launch(t) for t in STEPS] + [value_launch(3, OTHER_BETAS)]


def clamp_values(c):
    """g of the clamp battery: +-c, one ulp inside, one ulp outside, +-inf, NaN, -NaN, and a few ordinary values (16 in all)"""
    c = np.float32(c)
    inside, outside = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(np.inf))
    nan = np.float32(np.nan)
    g = np.array([c, -c, inside, -inside, outside, -outside, np.inf, -np.inf, nan, -nan, 0.5, -0.5, 2.0, -3.0, 0.0, 0.25], dtype=np.float32)
    g.view(np.uint32)[9] |= 0x80000000        # -NaN: the sign bit set whatever numpy's negation made of it
    g.view(np.uint32)[8] &= 0x7FFFFFFF
    return torch.from_numpy(g)


@functools.lru_cache(maxsize=None)
def clamp_launch(clip):
    """three records at t = 4: the 16 values on the vector path, the same rolled by two (so that every special value meets
    every lane position of a float4 between the two), and 15 of them on the scalar path.  clip None: no clipping; the edge
    values are then those of +-1."""
    vals = clamp_values(clip or 1.0)
    recs = []
    for k, (n, roll) in enumerate(((16, 0), (16, 2), (15, 0))):
        r = record(n, 1.0, 4, key=("clamp", k))
        r["g"] = torch.roll(vals, roll)[:n].clone()
        recs.append(r)
    return dict(t=4, betas=BETAS, eps=EPS, clip=clip, records=recs)


LENGTHS = (1, 2, 3, 4, 5, 8, 255, 256, 1023, 1024, 1025, 1028, 8188, 8191, 8192, 8193, 8196, 16384, 16388, 24580)
OFFSET_LENGTHS = (8, 1028, 8192, 16388)


@functools.lru_cache(maxsize=None)
def layout_launch():
    """t = 7.  Every length of LENGTHS with all streams aligned; every length of OFFSET_LENGTHS (n % 4 == 0) with ONE stream
    at a time -- p, g, m, v by 1, 2 and 3 floats, the shadow by 1, 2 and 3 bf16 elements -- off its alignment.  Every third
    aligned record has no shadow; (lr, wd) cycles through LR_WD (wd = 0 and lr = 0 among them); the gradient scale cycles
    through 1, 1e-4, 1e-8."""
    specs = [(n, None) for n in LENGTHS] + [(n, {k: o}) for n in OFFSET_LENGTHS for k in "pgmvs" for o in (1, 2, 3)]
    recs = []
    for i, (n, off) in enumerate(specs):
        lr, wd = LR_WD[i % 3]
        recs.append(record(n, SCALES[i % 3], 7, lr=lr, wd=wd, shadow=bool(off) or i % 3 != 2, off=off, key=("layout", i)))
    return dict(t=7, betas=BETAS, eps=EPS, clip=None, records=recs)


def place(records):
    """where each record's tensors start in the five arenas (fp32 p, g, m, v; bf16 s), in elements: every tensor starts
    record["off"][k] elements past a multiple of 4 (16 bytes of fp32, 8 bytes of bf16) and has at least GAP canary elements
    before and after it.  Returns ([{"p": start, ...} per record; "s" None without a shadow], {arena: size})."""
    cur = dict.fromkeys("pgmvs", 0)
    at = []
    for r in records:
        a = {}
        for k in "pgmvs":
            if k == "s" and not r["shadow"]:
                a[k] = None
                continue
            a[k] = cur[k] + GAP + r["off"][k]
            cur[k] = (a[k] + r["n"] + 3) // 4 * 4
        at.append(a)
    return at, {k: cur[k] + GAP for k in "pgmvs"}


def chunk_list(records, shuffled=False):
    """int32 (n_chunks, 2) {record, chunk} pairs in table order, or in a seeded random order"""
    ch = np.array([(i, c) for i, r in enumerate(records) for c in range((r["n"] + CHUNK - 1) // CHUNK)], dtype=np.int32).reshape(-1, 2)
    if shuffled:
        ch = ch[np.random.default_rng(5).permutation(len(ch))]
    return ch


SWEEP_HIGH = (0x3F80, 0x3F81, 0xBF80, 0xC2FF, 0x7F7F, 0x0080)


def sweep_values(high):
    """the 65536 fp32 numbers whose upper half is `high` (sign, exponent, seven mantissa bits): every low-half bit pattern,
    the ties 0x8000 to an even (0x3F80, 0xBF80, 0x0080) and to an odd (0x3F81, 0xC2FF, 0x7F7F) neighbour included; 0xC2FF
    carries into the exponent when it rounds up, 0x7F7F (the largest finite numbers) rounds up to infinity, 0x0080 is the
    smallest normal binade"""
    bits = (np.int64(high) << 16) + np.arange(65536, dtype=np.int64)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())
