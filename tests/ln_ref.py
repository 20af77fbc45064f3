"""Reference, bound and inputs of the row kernels of csrc/ln.hip and csrc/ln_bwd_kernel_body.h (fused dropout + stochastic
depth + residual + LayerNorm forward / backward, one or two row groups, the stored-sum backward, the deterministic backward) and
of gelu_fwd_kernel, for tests/test_ln_bound_cpu.py and tests/test_ln_bound_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  fp64 from the bf16 operands the kernel sees.  The keep mask (ln_keep), the drop-path mask (ln_path_scale) and the
seed mix (ln_seed) are restated in 64-bit integer tensors masked to 32 bits; thresholds and scales are formed as the launcher
forms them: p is a C float, thresh = (unsigned)((double)p * 2^32), inv_keep = 1.0f / (1.0f - p) in fp32.
    xs = x keep inv_keep ps,   z = xs + residual                      (the stored-sum backward: z = s)
    forward    mean, var over the row, rstd = (var + eps)^-1/2, zhat = (z - mean) rstd, y = zhat gamma + beta, sum = z
    backward   takes mean and rstd as GIVEN fp32 values (the kernel reads them): zhat = (z - mean) rstd,
               gd = dy gamma, s1 = mean_j gd, s2 = mean_j gd zhat, dz = rstd (gd - s1 - zhat s2) + dsum,
               dres = dz, dx = dz ps keep inv_keep, dgamma = sum_rows dy zhat, dbeta = sum_rows dy   (per row group)

BOUND, per element.  u = 2^-24 (fp32 round to nearest), Hu = (H + 8) u: a sum of H fp32 terms in ANY order errs by at most
(H - 1) u sum|terms| to first order (the kernel's order -- 4 NCH serial adds per lane, then the DPP wave sum -- is far shorter;
the bound does not depend on it), and 8 covers the handful of elementwise roundings around each sum.  mean_j / rms_j run over
the row.  The rounding points, in kernel order:

  z     x inv_keep, then ps, then + residual: one rounding each where the factor is not 1:
            e_z = n u |xs| + u |z|,  n = (p_drop > 0) + (p_path > 0);     az = |xs| + |residual| >= |z|, e_z <= 3 u az
  mean  H-term sum of z, one division:                e_mean = Hu mean_j az
  rstd  d = z - mean (1 rounding), d d (1), H-term sum, / H (1), + eps (1), rsqrtf (1 ulp = 2 u).  An error dm of the mean
        enters the variance only as dm^2 (sum_j d_j = 0), an error dz_j of z as 2 d_j dz_j:
            |d var| / (var + eps) <= (H + 4) u + 2 rstd rms_j(e_z) + rstd^2 (e_mean + max_j e_z)^2
        (Cauchy-Schwarz and sigma rstd <= 1), and rstd takes half of the first-order part plus 2 u:
            rel_rstd = Hu + 3 u rstd rms_j az + (rstd (e_mean + max_j e_z))^2
        The last, second-order, term is negligible except where rstd is huge: a constant row (var = 0, rstd = eps^-1/2), where the
        bound is loose by construction.
  zhat  (z - mean) rstd: two roundings:               e_zhat = rstd (e_z + e_mean) + |zhat| (rel_rstd + 2 u)
  y     zhat gamma + beta: two roundings:             e_y = |gamma| e_zhat + u |zhat gamma| + u |y|
  sum   z itself:                                     e_sum = e_z
  every bf16 output: 2^-8 (|r| + e) + e, as gemm_ref.bound (bf16 keeps 8 significant bits).
  mean and rstd are fp32 outputs: e_mean and rstd rel_rstd alone.

The issue's table writes e_zhat as H u (|zhat| + rstd (mean|z| + |z|)): the terms are the same, but here the error of z is carried
as the 3 u it is instead of H u (|z| was standing in for it), and |z| is replaced by az where x and the residual cancel -- az is
what the roundings are relative to.  The rstd term 3 u rstd rms az is new: it is the first-order effect of e_z on the variance,
which for a row of mean 40 and unit variance (120 u) is as large as the summation term at H = 256.

  backward, mean and rstd given (exact in the reference too); z re-formed as in the forward (e_z; 0 for the stored sum):
  zhat  e_zh = rstd e_z + 2 u |zhat|
  gd    one rounding, u |gd|
  s1    e_s1 = Hu mean_j |gd|                       s2    e_s2 = Hu mean_j |gd zhat| + mean_j |gd| e_zh
  t = gd - s1 - zhat s2, A = |gd| + |s1| + |zhat s2|:  e_t = 3 u A + e_s1 + |zhat| e_s2 + |s2| e_zh
  dz = rstd t + dsum:                                 e_dz = rstd (e_t + u A) + u |dz|
  dres  bf16 of dz;  dx = dz ps inv_keep (two more roundings): e_dx = ps keep inv_keep (e_dz + 2 u |dz|), then bf16;
        where the mask or the path drops, dx is 0 and the tolerance is 0.
  dgamma  (Mg + 8) u sum_rows |dy zhat| + sum_rows |dy| e_zh     (Mg rows of the group added in any order -- registers, the
  dbeta   (Mg + 8) u sum_rows |dy|                                4-wave fold, atomics or the slab fold; fp32 outputs)
The issue's e_dz has the same terms under a common factor 2 H u; here each carries its own constant.

GELU.  Reference gemm_ref.gelu_erf in fp64 at the bf16 input; tolerance 2^-8 |r| + 4 u |x| (the second term: a few u of error in
1 + erff(x / sqrt 2) times 0.5 |x|).  One amendment: where |r| < 2^-126 the RESULT is a bf16 subnormal, which does not keep 8
significant bits -- its spacing is 2^-133 whatever its size, so a correctly rounded result errs by up to 2^-134 (x = 2^-133 has
r = 2^-134, a tie) and fails the tolerance as stated.  There, and only there, 2^-134 is added (gelu_bound).
"""
import functools
import zlib

import torch

from gemm_ref import gelu_erf

U = 2.0 ** -24
B8 = 2.0 ** -8
MASK32 = 0xFFFFFFFF
FWD_CAP, BWD_CAP = 1024, 384          # csrc/ln.hip: BQ_LN_FWD_CAP, ln_bwd_blocks


# ---- the hashes of csrc/ln.hip, restated ----------------------------------------------------------------------------------------
def _mix(h):
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & MASK32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & MASK32
    return h ^ (h >> 16)


def _hash(seed, row, col):
    """ln_keep's 32-bit value for int64 tensors row, col (broadcast)"""
    return _mix((seed & MASK32) ^ ((row * 0x85EBCA77) & MASK32) ^ ((col * 0xC2B2AE3D) & MASK32))


def eff_seed(seed, seed_value=None):
    """ln_seed: seed_value = the content of the seed tensor (an int32 read as unsigned), or None"""
    seed &= MASK32
    return seed if seed_value is None else ((seed_value & MASK32) * 2654435761 + seed) & MASK32


def thresh(p):
    """(unsigned)((double)p * 2^32) of the C float p"""
    return int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0)


def inv_keep(p):
    """1.0f / (1.0f - p) in fp32, as a Python float"""
    one = torch.tensor(1.0, dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


def keep_mask(seed, M, H, p, row0=0):
    """bool (M, H): True where ln_keep keeps element (row0 + r, c)"""
    r = torch.arange(row0, row0 + M, dtype=torch.int64).view(M, 1)
    c = torch.arange(H, dtype=torch.int64).view(1, H)
    return _hash(seed, r, c) >= thresh(p)


def path_keep(seed, M, p_path, rows_per_sample):
    """bool (M,): True where ln_path_scale keeps the row's sample"""
    sample = torch.arange(M, dtype=torch.int64) // rows_per_sample
    return _hash(seed ^ 0x5BD1E995, sample, torch.tensor(0x3039, dtype=torch.int64)) >= thresh(p_path)


def masks(M, H, p_drop=0.0, p_path=0.0, rows_per_sample=0, seed=0, seed_value=None):
    """(kscale, ps): keep inv_keep as fp64 (M, H) and the path scale as fp64 (M,), each None where its p is 0"""
    s = eff_seed(seed, seed_value)
    kscale = keep_mask(s, M, H, p_drop).double() * inv_keep(p_drop) if p_drop > 0 else None
    ps = path_keep(s, M, p_path, rows_per_sample).double() * inv_keep(p_path) if p_path > 0 else None
    return kscale, ps


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=4)
def inputs(M, H, tag=0):
    """dict of x, res, dy, dsum (bf16 (M, H)), gamma, beta, gamma2, beta2 (f32 (H,)), seeded by the shape.  x ~ 2 N(0, 1),
    res ~ 3 N(0, 1) + 0.5; row 1 has mean 40 and unit variance, row 2 is scaled by 24, row 3 is constant (z = 2 exactly
    without dropout); gamma in [0.5, 1.5] with gamma[5] = 0 and gamma[H - 3] = -0.75; gamma2 / beta2 differ clearly.
    Shared between tests: do not write to the tensors."""
    g = torch.Generator().manual_seed(_seed("ln", M, H, tag))
    x = torch.randn(M, H, generator=g) * 2.0
    res = torch.randn(M, H, generator=g) * 3.0 + 0.5
    if M > 1:
        x[1] = torch.randn(H, generator=g) + 40.0
        res[1] = torch.randn(H, generator=g) * 0.25
    if M > 2:
        x[2] *= 24.0
        res[2] *= 24.0
    if M > 3:
        x[3] = 1.5
        res[3] = 0.5
    dy = torch.randn(M, H, generator=g)
    dsum = torch.randn(M, H, generator=g)
    gamma = torch.rand(H, generator=g) + 0.5
    gamma[5], gamma[H - 3] = 0.0, -0.75
    beta = torch.randn(H, generator=g) * 0.1
    gamma2 = torch.rand(H, generator=g) + 0.5                      # independent of gamma: they differ by 1/3 on average
    beta2 = torch.randn(H, generator=g) * 0.1 + 0.5
    bf = lambda t: t.to(torch.bfloat16)
    return dict(x=bf(x), res=bf(res), dy=bf(dy), dsum=bf(dsum), gamma=gamma, beta=beta, gamma2=gamma2, beta2=beta2)


SPECIAL_ROWS = (1, 2, 3)


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def _z(x, res, kscale, ps):
    """(xs, z, e_z, az) in fp64"""
    xs = x.double()
    n = 0
    if kscale is not None:
        xs, n = xs * kscale, n + 1
    if ps is not None:
        xs, n = xs * ps[:, None], n + 1
    r = res.double() if res is not None else torch.zeros_like(xs)
    z = xs + r
    return xs, z, n * U * xs.abs() + U * z.abs(), xs.abs() + r.abs()


def _bf16_tol(r, e):
    return B8 * (r.abs() + e) + e


def forward(x, res, gamma, beta, eps, kscale=None, ps=None):
    """fp64 z, mean, rstd, zhat, y and the tolerances tol_y, tol_sum (bf16 outputs), tol_mean, tol_rstd (fp32 outputs), plus
    e_y / e_sum (their fp32 parts)"""
    H = x.shape[1]
    Hu = (H + 8) * U
    eps = float(torch.tensor(eps, dtype=torch.float32))
    g, b = gamma.double(), beta.double()
    xs, z, e_z, az = _z(x, res, kscale, ps)
    mean = z.mean(1, keepdim=True)
    d = z - mean
    rstd = (d.square().mean(1, keepdim=True) + eps).rsqrt()
    zhat = d * rstd
    y = zhat * g + b
    e_mean = Hu * az.mean(1, keepdim=True)
    rel_rstd = (Hu + 3.0 * U * rstd * az.square().mean(1, keepdim=True).sqrt()
                + (rstd * (e_mean + e_z.amax(1, keepdim=True))).square())
    e_zhat = rstd * (e_z + e_mean) + zhat.abs() * (rel_rstd + 2.0 * U)
    e_y = g.abs() * e_zhat + U * (zhat * g).abs() + U * y.abs()
    return dict(z=z, mean=mean[:, 0], rstd=rstd[:, 0], zhat=zhat, y=y, e_y=e_y, e_sum=e_z,
                tol_y=_bf16_tol(y, e_y), tol_sum=_bf16_tol(z, e_z), tol_mean=e_mean[:, 0], tol_rstd=(rstd * rel_rstd)[:, 0])


def backward(x, res, gamma, dy, dsum, mean, rstd, kscale=None, ps=None, x_is_sum=False):
    """fp64 dz (= dres), dx, dgamma, dbeta with tol_dres, tol_dx (bf16), tol_dgamma, tol_dbeta (fp32) and e_dz, for ONE row
    group.  mean, rstd: the fp32 tensors the kernel is given.  x_is_sum: x is the stored bf16 sum (no dropout, no residual; the
    path scale reaches dx only)."""
    M, H = x.shape
    Hu, Mu = (H + 8) * U, (M + 8) * U
    g, dyd = gamma.double(), dy.double()
    if x_is_sum:
        z = x.double()
        e_z = torch.zeros_like(z)
    else:
        _, z, e_z, _ = _z(x, res, kscale, ps)
    m, rs = mean.double()[:, None], rstd.double()[:, None]
    zhat = (z - m) * rs
    e_zh = rs * e_z + 2.0 * U * zhat.abs()
    gd = dyd * g
    s1 = gd.mean(1, keepdim=True)
    s2 = (gd * zhat).mean(1, keepdim=True)
    e_s1 = Hu * gd.abs().mean(1, keepdim=True)
    e_s2 = Hu * (gd * zhat).abs().mean(1, keepdim=True) + (gd.abs() * e_zh).mean(1, keepdim=True)
    A = gd.abs() + s1.abs() + (zhat * s2).abs()
    e_t = 3.0 * U * A + e_s1 + zhat.abs() * e_s2 + s2.abs() * e_zh
    dz = rs * (gd - s1 - zhat * s2)
    if dsum is not None:
        dz = dz + dsum.double()
    e_dz = rs * (e_t + U * A) + U * dz.abs()
    sc = torch.ones_like(dz)
    if kscale is not None:
        sc = sc * kscale
    if ps is not None:
        sc = sc * ps[:, None]
    dx = dz * sc
    e_dx = sc * (e_dz + 2.0 * U * dz.abs())
    tol_dx = torch.where(sc == 0, torch.zeros_like(dx), _bf16_tol(dx, e_dx))
    dyz = dyd * zhat
    return dict(dz=dz, dx=dx, e_dz=e_dz, tol_dres=_bf16_tol(dz, e_dz), tol_dx=tol_dx, dropped=(sc == 0),
                dgamma=dyz.sum(0), dbeta=dyd.sum(0),
                tol_dgamma=Mu * dyz.abs().sum(0) + (dyd.abs() * e_zh).sum(0), tol_dbeta=Mu * dyd.abs().sum(0))


def stats32(z, eps):
    """mean and rstd of the fp64 rows z, rounded once to fp32: what a backward-only test hands to the kernel AND to the
    reference"""
    mean = z.mean(1, keepdim=True)
    var = (z - mean).square().mean(1)
    return mean[:, 0].float(), (var + eps).rsqrt().float()


def gelu_bound(x):
    """(r, tol) of gelu at the bf16 tensor x"""
    xd = x.double()
    r = gelu_erf(xd)
    tol = B8 * r.abs() + 4.0 * U * xd.abs()
    return r, torch.where(r.abs() < 2.0 ** -126, tol + 2.0 ** -134, tol)


def finite_bf16_patterns():
    """every finite bf16 value, by bit pattern (65280 of them, +0 first and -0 at index 32640)"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return v[torch.isfinite(v.float())].contiguous()


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def excess(out, ref, tol):
    """(worst |err| / tol over the elements with tol > 0, message or None).  `not (err <= tol)` fails, so NaN fails; the message
    gives the count, the worst excess and the index of the first offender."""
    out = out.detach().cpu().double().reshape(ref.shape)
    err = (out - ref).abs()
    bad = ~(err <= tol)
    held = tol > 0
    ratio = float((err[held] / tol[held]).max()) if held.any() else 0.0
    if not bad.any():
        return ratio, None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    worst = float((err - tol)[bad].nan_to_num(nan=float("inf")).max())
    return float("inf") if ratio != ratio else ratio, "%d of %d out of bound, worst excess %.3e (|err| / tol up to %.3g), first at %s: out %r ref %r tol %.3e" % (
        int(bad.sum()), out.numel(), worst, ratio, idx, float(out[idx]), float(ref[idx]), float(tol[idx]))


# ---- the whole-tensor norms of tests/test_attn_gpu.py, restated (what the planted defects must still pass) ------------------------
def old_norms_accept(out, ref, grad=False):
    """test_fused_dropout_add_layernorm_fwd_bwd and its siblings: rel-L2 < 1e-2 for y and the sum, < 2e-2 for the gradients"""
    out, ref = out.float(), ref.float()
    rel = ((out - ref).norm() / ref.norm()).item()
    return bool(torch.isfinite(out).all()) and rel < (2e-2 if grad else 1e-2)


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------
def _wave_sum(v):
    """row sums of fp32 (M, H) as one wave forms them: lane l owns columns ch 256 + 4 l + j and adds its 4 NCH values serially
    (i = 4 ch + j), then the 64 lane sums are folded as a tree"""
    M, H = v.shape
    t = v.view(M, H // 256, 64, 4).permute(0, 2, 1, 3).reshape(M, 64, H // 64)
    s = torch.zeros(M, 64, dtype=torch.float32)
    for i in range(t.shape[2]):
        s = s + t[:, :, i]
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s


def _z32(x, res, kscale, ps):
    v = x.float()
    if kscale is not None:
        v = v * kscale.float()
    if ps is not None:
        v = v * ps.float()[:, None]
    return v + res.float() if res is not None else v


def emulate_forward(x, res, gamma, beta, eps, kscale=None, ps=None):
    """y, sum (bf16), mean, rstd (fp32) with the kernel's rounding points"""
    H = x.shape[1]
    z = _z32(x, res, kscale, ps)
    mean = _wave_sum(z) / float(H)
    d = z - mean
    rstd = torch.rsqrt(_wave_sum(d * d) / float(H) + torch.tensor(eps, dtype=torch.float32))
    y = (z - mean) * rstd * gamma.float() + beta.float()
    return y.to(torch.bfloat16), z.to(torch.bfloat16), mean[:, 0], rstd[:, 0]


def emulate_backward(x, res, gamma, dy, dsum, mean, rstd, kscale=None, ps=None, x_is_sum=False):
    """dx, dres (bf16), dgamma, dbeta (fp32): rows strided over min(ceil(M / 4), 384) workgroups of 4 waves, every wave adding
    its rows in order, the 4-wave fold, then the workgroups' partials added in workgroup order"""
    M, H = x.shape
    z = x.float() if x_is_sum else _z32(x, res, kscale, ps)
    m, rs = mean.float()[:, None], rstd.float()[:, None]
    g, dyf = gamma.float(), dy.float()
    zhat = (z - m) * rs
    gd = dyf * g
    invH = torch.tensor(1.0, dtype=torch.float32) / float(H)
    s1 = _wave_sum(gd) * invH
    s2 = _wave_sum(gd * zhat) * invH
    dz = rs * (gd - s1 - zhat * s2)
    if dsum is not None:
        dz = dz + dsum.float()
    dxv = dz * ps.float()[:, None] if ps is not None else dz
    if kscale is not None:
        dxv = dxv * kscale.float()
    blocks = min((M + 3) // 4, BWD_CAP)
    slots = blocks * 4
    ag = torch.zeros(slots, H, dtype=torch.float32)
    ab = torch.zeros(slots, H, dtype=torch.float32)
    for r0 in range(0, M, slots):
        n = min(slots, M - r0)
        ag[:n] = ag[:n] + dyf[r0:r0 + n] * zhat[r0:r0 + n]
        ab[:n] = ab[:n] + dyf[r0:r0 + n]
    ag, ab = ag.view(blocks, 4, H), ab.view(blocks, 4, H)
    pg = (ag[:, 0] + ag[:, 1]) + (ag[:, 2] + ag[:, 3])
    pb = (ab[:, 0] + ab[:, 1]) + (ab[:, 2] + ab[:, 3])
    dg, db = torch.zeros(H, dtype=torch.float32), torch.zeros(H, dtype=torch.float32)
    for k in range(blocks):
        dg, db = dg + pg[k], db + pb[k]
    return dxv.to(torch.bfloat16), dz.to(torch.bfloat16), dg, db
