"""Reference, bound and inputs of the training-mode BatchNorm kernels of csrc/bn.hip (bn_stats_kernel, bn_finalize_kernel,
bn_fold_kernel, bn_apply_kernel<RELU, POOL>, bn_bwd_reduce_kernel, bn_bwd_dx_kernel) and of bn_bwd_reduce_arg_kernel
(csrc/detbwd.hip), for tests/test_bn_bound_cpu.py and tests/test_bn_bound_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  fp64 from the bf16 operands the kernels see; x is (R, C) point-major, everything below is per channel.
    statistics  p = x[0, c] (the pivot), t = x - p, dm = mean_r t, q = mean_r t^2, mean = p + dm, var = max(q - dm^2, 0),
                rstd = (var + eps)^-1/2, scale = gamma rstd, shift = beta - mean scale; running_mean <- (1 - m) rm + m mean,
                running_var <- (1 - m) rv + m var R / (R - 1) (plain var when R = 1); eps and m are the C floats the launcher gets
    apply       scale, shift GIVEN (fp32): z = x scale + shift, y = bf16(relu?(z)) or y[g] = bf16(relu?(max_s z[g S + s])),
                arg[g] = the FIRST s attaining the maximum
    backward    scale, shift, mean, rstd GIVEN: g = dy [z > 0] under ReLU (strict); pooled: the group's dy goes to its arg row
                only (and only if that row's z > 0 under ReLU), every other row has g = 0; xhat = (x - mean) rstd,
                dbeta = sum_r g, dgamma = sum_r g xhat, dx = scale (g - dbeta / R - xhat dgamma / R) on EVERY row (R = the row
                count, also when pooled)

BOUND.  u = 2^-24, Du = (D + 8) u with D the longest chain of dependent adds a term passes through: a sum formed as a tree of
depth D errs by at most D u sum|terms| to first order, whatever the order inside that depth; 8 covers the elementwise roundings
around each sum (x - p, the square or product -- contracted or not --, 1 / R and the product with it).  depth() restates D from
the kernels' chunking and never assumes less than they do: cr = 256 rows per partial (1024 from R = 2^20), rps = 2048 / C row
phases, n_t = ceil(cr / rps) serial adds per thread, rps phase adds, then the fold of the n_c partials:
    D = n_t + rps + max(ceil(n_c / 4), F), capped at the number of terms,
F = the fold's own chain of inexact adds (an add onto 0 is exact): a phase holds k = ceil(n_c / P) partials; its unrolled trips
add k div 8 per accumulator, its tail k mod 8 onto the first, the accumulator tree 3 (none when no trip ran); the P phase sums
are added as a tree of 2 (fold_column, P = 4, statistics) or in order, min(n_c, 16) - 1 adds (bn_fold_kernel, P = 16, backward).
Pooled reductions: cr is replaced by the groups per chunk max(cr / S, 1); the table-reading reduce has gps = 256 / C phases and
ceil(G / n_c) groups per chunk.

  statistics   e_dm = Du mean_r|t|;  e_mean = e_dm + u |mean|;  e_var = Du q + 2 |dm| e_dm + 3 u (q + dm^2);
               r = e_var / (var + eps), rel_rstd = r / (2 (1 - r)) + 3 u  (var + eps: 1 rounding, halved; rsqrtf: 1 ulp = 2 u);
               e_scale = |scale| (rel_rstd + u);  e_shift = |mean| e_scale + |scale| e_mean + u |mean scale| + u |shift|
               running_mean: (1 - m) e_prev + m e_mean + 3 u (|(1 - m) rm| + |m mean|)     (e_prev: the error rm came with)
               running_var:  (1 - m) e_prev + m e_unb  + 3 u (|(1 - m) rv| + |m unb|),  e_unb = e_var R / (R - 1) + 2 u unb
  apply        e_z = u |x scale| + u |z| (covers the contracted and the uncontracted form), and e_z = 0 where both x scale and z
               are fp32 numbers: nothing is rounded then, in either form.  relu and max are 1-Lipschitz: pooled e = max_s e_z;
               under ReLU e = 0 where z < -e_z (the output is exactly 0).  Every bf16 output: tol = 2^-8 (|r| + e) + e.
  backward     e_xh = 2 u |xhat|;  tol_dbeta = Du sum|g|;  tol_dgamma = Du sum|g xhat| + sum|g| e_xh;
               mb = dbeta / R, e_mb = tol_dbeta / R + 2 u |mb| (1 / R and the product; the kernel divides its OWN sums), mg alike;
               A = |g| + |mb| + |xhat mg|,  e_t = 3 u A + e_mb + |xhat| e_mg + |mg| e_xh,  e_dx = |scale| (e_t + u A), then bf16.

Against the issue's table: (1) rel_rstd is written r / (2 (1 - r)) instead of r / 2 -- (1 - r)^-1/2 - 1 <= r / (2 (1 - r)) holds
for every r < 1, the first-order form only for small r; r < 1/2 is asserted, and on the inputs here the two differ by < 1e-4
relative.  (2) the fold term of D is max(ceil(n_c / 4), F), not ceil(n_c / 4) alone: for few partials the
issue's term is less than the kernels' chain -- bn_fold_kernel adds its 16 phase sums in order, so 34 partials make 2 + 15
adds against ceil(34 / 4) = 9, and fold_column makes 6 + 2 at 28 partials against 7; from ~100 partials on
ceil(n_c / 4) is the larger and nothing changes.  (3) e_z is 0 where no rounding can happen (above): this is
what makes the exact-arithmetic channels DECIDED with tolerance 0, as the issue requires of them, and it also covers gamma = 0
(scale = 0: every z is the fp32 shift itself).  (4) e = 0 under ReLU where z < -e_z: sharper than the Lipschitz argument alone.
(5) the second-order effect of an undecided element on sum|g| is included by counting |dy| there.  Nothing else differs.

UNDECIDED ELEMENTS (conditions, not tolerances).  ReLU mask: an element with |z| <= e_z and e_z > 0 may be masked either way; its
dx tolerance gains |scale dy|, its channel's dbeta / dgamma tolerances gain |dy| / |dy xhat|; backward() asserts that at most 1e-4
of a case's elements are undecided.  Arg-max: a group is contested when a row with a DIFFERENT x value lies within 2 max_s e_z of
the maximum (and any rounding happens at all in the group: with e_z = 0 throughout, the comparison is exact); apply() and
backward() assert that there is none, so every arg byte and every routed gradient is compared exactly as decided.  Rows with the
same x are exact ties in the kernel: the first wins, here too.
"""
import functools
import zlib

import torch

from ln_ref import excess  # noqa: F401  (the comparison of the test modules)

U = 2.0 ** -24
B8 = 2.0 ** -8
WIDTHS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)
UNDECIDED_CAP = 1e-4
# channels 0 .. 7 of every input (C >= 8): 0 ordinary, 1 mean 40 / std 0.5, 2 constant, 3 scaled by 24, 4 and 7 carry exact
# arithmetic under given_stats (scale a power of two, shift exact in bf16), 5 gamma = 0, 6 gamma = -0.75
CH_MEAN40, CH_CONST, CH_BIG, CH_EXACT_A, CH_GAMMA0, CH_GAMMA_NEG, CH_EXACT_B = 1, 2, 3, 4, 5, 6, 7
SPECIAL_CHANNELS = (1, 2, 3, 4, 5, 6, 7)
EXACT = {CH_EXACT_A: (0.5, 0.40625), CH_EXACT_B: (2.0, -1.25)}      # channel: (scale, the x value v with z(v) = 0)
SENTINEL = 64.0


def _cdiv(a, b):
    return -(-a // b)


# ---- the chunking of csrc/bn.hip, restated ----------------------------------------------------------------------------------------
def chunk_rows(R):
    """bn_chunk_rows"""
    return 1024 if R >= (1 << 20) else 256


def layout(R, C, S=0, pool=False, table=False):
    """(n, per, ph, n_c): the terms of a reduction, terms per partial, phases per partial, partials.  pool: the terms are the
    R / S groups; table: bn_bwd_reduce_arg_kernel (C <= 256)"""
    cr = chunk_rows(R)
    n, per, ph = (R // S, max(cr // S, 1), 2048 // C) if pool else (R, cr, 2048 // C)
    n_c = _cdiv(n, per)
    if table:
        per, ph = _cdiv(n, n_c), 256 // C
    return n, per, ph, n_c


def fold_depth(n_c, phases):
    """the longest chain of adds a partial passes through in fold_column (phases = 4) or bn_fold_kernel (phases = 16)"""
    def chain(k):      # an add onto 0 is exact: the first of an accumulator, and the whole accumulator tree when no trip ran
        trips, tail = k // 8, k % 8
        return trips - 1 + tail + 3 if trips else max(tail - 1, 0)
    return max(chain(_cdiv(n_c, phases)), chain(max(n_c // phases, 1))) + (min(n_c - 1, 2) if phases == 4 else min(n_c, 16) - 1)


def depth(R, C, S=0, pool=False, table=False, backward=False):
    """(D, n_c); backward (and every pooled or table-reading reduction, which are the backward's): the partials are folded by
    bn_fold_kernel, else (the statistics) by fold_column"""
    n, per, ph, n_c = layout(R, C, S, pool, table)
    phases = 16 if (backward or pool or table) else 4
    return max(1, min(_cdiv(per, ph) + ph + max(_cdiv(n_c, 4), fold_depth(n_c, phases)), n)), n_c


def sentinel_positions(n, per):
    """the last term, the first of the last partial, the last of the first partial and term 1 (the second phase of the first
    partial); never term 0 (the pivot row)"""
    n_c = _cdiv(n, per)
    return sorted(r for r in {n - 1, (n_c - 1) * per, min(per, n) - 1, 1} if 0 < r < n)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _bf(t):
    return t.to(torch.bfloat16)


@functools.lru_cache(maxsize=3)
def inputs(R, C, S=0, tag=0):
    """dict of x bf16 (R, C), dy bf16 (R, C) -- or (R / S, C) when S > 0: a pooled case --, gamma, beta, rm, rv f32 (C).
    x ~ 1.5 N(0, 1) + a per-channel offset; the special channels as listed above; x (not its channels 1 and 2) and dy get +-64 on
    the sentinel rows (dy of a pooled case: on the sentinel groups).  Pooled cases with S >= 2 plant ties: in a fifth of the
    (group, channel) pairs of the channels that are not 2, 4, 5, 7 two or three rows hold the group's extreme value (the maximum,
    under gamma < 0 the minimum) bit for bit, and a third of those pairs lie 6 sigma below (above) the rest of the channel, so
    that their maximum has z < 0; channels 4 and 7 hold their value v at the first eight rows that are 5 mod 11 / 6 mod 13, and every
    seventh group is clamped to <= v with v at two rows: a tie whose z is exactly 0.  tag = "plain": no sentinels (the planted
    defects of the CPU test: a sentinel would make a dropped row loud in the old norms too).  Shared between tests: do not write
    to the tensors."""
    assert C in WIDTHS and R >= 1 and (S == 0 or R % S == 0)
    gen = torch.Generator().manual_seed(_seed("bn", R, C, S, tag))
    off = torch.randn(C, generator=gen) * 0.5
    x = torch.randn(R, C, generator=gen) * 1.5 + off
    x[:, CH_MEAN40] = torch.randn(R, generator=gen) * 0.5 + 40.0
    x[:, CH_CONST] = 1.5
    x[:, CH_BIG] *= 24.0
    n_dy = R // S if S else R
    dy = torch.randn(n_dy, C, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[CH_GAMMA0], gamma[CH_GAMMA_NEG] = 0.0, -0.75
    beta = torch.randn(C, generator=gen) * 0.1
    beta = beta + torch.where(beta < 0, -0.03, 0.03)   # |beta| >= 0.03: a constant channel (and every channel at R = 1) has z = beta
    beta[CH_CONST], beta[CH_GAMMA0] = 0.25, 0.125      # every z of these channels equals beta: keep it clear of 0
    rm = torch.randn(C, generator=gen) * 0.3
    rv = torch.rand(C, generator=gen) + 0.5
    sign = 1.0 - 2.0 * (torch.arange(C) % 2)
    xs_sign = sign.clone()
    xs_sign[CH_MEAN40] = xs_sign[CH_CONST] = 0.0
    amp = 0.0 if tag == "plain" else SENTINEL
    for k, r in enumerate(sentinel_positions(R, chunk_rows(R))):
        x[r] += amp * xs_sign * (-1.0) ** k
    per_dy = layout(R, C, S, True)[1] if S else chunk_rows(R)
    for k, r in enumerate(sentinel_positions(n_dy, per_dy)):
        dy[r] += amp * sign * (-1.0) ** k
    sgn = torch.ones(C)
    sgn[CH_GAMMA_NEG] = -1.0
    tied = None
    if S >= 2:
        G = R // S
        gi, ci = torch.meshgrid(torch.arange(G), torch.arange(C), indexing="ij")
        tied = (gi * 7 + ci * 3) % 5 == 0
        for c in (CH_CONST, CH_EXACT_A, CH_GAMMA0, CH_EXACT_B):
            tied[:, c] = False
        low = tied & ((gi + ci) % 3 == 0)
        sigma = torch.full((C,), 1.5)
        sigma[CH_MEAN40], sigma[CH_BIG] = 0.5, 36.0
        xv = x.view(G, S, C)
        xv -= (low * (6.0 * sigma * sgn))[:, None, :]
    x = _bf(x).float()
    for c, (_, v) in EXACT.items():
        step = 11 if c == CH_EXACT_A else 13
        rows = torch.arange(R)[step // 2::step][:8]
        x[rows, c] = v
    if S >= 2:
        xv = x.view(G, S, C)
        ext = (xv * sgn).amax(1) * sgn                             # (G, C): the group's extreme value
        g_, c_ = tied.nonzero(as_tuple=True)
        p1 = (3 * g_ + c_) % S
        p2 = (p1 + 1 + g_ % (S - 1)) % S
        p3 = torch.where(g_ % 2 == 0, (p1 + S // 2 + 1) % S, p2)
        for p in (p1, p2, p3):
            xv[g_, p, c_] = ext[g_, c_]
        gz = torch.arange(G)[3::7]
        for c, (_, v) in EXACT.items():
            xv[gz, :, c] = xv[gz, :, c].clamp(max=v)
            xv[gz, gz % S, c] = v
            xv[gz, (gz + 1) % S, c] = v
    out = dict(x=_bf(x), dy=_bf(dy), gamma=gamma, beta=beta, rm=rm, rv=rv, tied=tied)
    assert torch.equal(out["x"].float(), x)
    return out


def stats32(x, eps):
    """mean and rstd of the bf16 x in fp64, rounded once to fp32"""
    xd = x.double()
    mean = xd.mean(0)
    var = (xd - mean).square().mean(0)
    return mean.float(), (var + _f32(eps)).rsqrt().float()


def given_stats(x, gamma, beta, eps=1e-5):
    """f32 (4, C) = scale | shift | mean | rstd as a backward-only or apply-only test hands them to the kernel AND to the
    reference: mean and rstd in fp64 rounded once (stats32), scale and shift formed from these in fp64 and rounded once; the two
    exact channels get scale 0.5 / 2 and shift = -scale v, so that z = scale (x - v) is exact in fp32 and 0 at x = v"""
    mean, rstd = stats32(x, eps)
    scale = gamma.double() * rstd.double()
    shift = beta.double() - mean.double() * scale
    st = torch.stack([scale.float(), shift.float(), mean, rstd])
    for c, (s, v) in EXACT.items():
        st[0, c], st[1, c] = s, -s * v
    return st


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def _bf16_tol(r, e):
    return B8 * (r.abs() + e) + e


def stats(x, gamma, beta, eps, momentum, rm=None, rv=None, e_rm=None, e_rv=None):
    """fp64 mean, var, rstd, scale, shift (and running_mean / running_var after one update of rm / rv, which came with the errors
    e_rm / e_rv) with their tolerances tol_*"""
    R, C = x.shape
    Du = (depth(R, C)[0] + 8) * U
    eps, m = _f32(eps), _f32(momentum)
    g, b = gamma.double(), beta.double()
    xd = x.double()
    p = xd[0]
    t = xd - p
    dm, q, at = t.mean(0), t.square().mean(0), t.abs().mean(0)
    mean = p + dm
    var = (q - dm * dm).clamp_min(0.0)
    rstd = (var + eps).rsqrt()
    scale = g * rstd
    shift = b - mean * scale
    e_dm = Du * at
    e_mean = e_dm + U * mean.abs()
    e_var = Du * q + 2.0 * dm.abs() * e_dm + 3.0 * U * (q + dm * dm)
    r = e_var / (var + eps)
    assert float(r.max()) < 0.5, "the variance bound is not small against var + eps"
    rel_rstd = 0.5 * r / (1.0 - r) + 3.0 * U
    e_scale = scale.abs() * (rel_rstd + U)
    e_shift = mean.abs() * e_scale + scale.abs() * e_mean + U * (mean * scale).abs() + U * shift.abs()
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, tol_mean=e_mean, tol_var=e_var, tol_rstd=rstd * rel_rstd,
               tol_scale=e_scale, tol_shift=e_shift)
    if rm is not None:
        unb = var * (R / (R - 1.0)) if R > 1 else var
        e_unb = (e_var * (R / (R - 1.0)) if R > 1 else e_var) + 2.0 * U * unb
        a0, a1 = (1.0 - m) * rm.double(), m * mean
        v0, v1 = (1.0 - m) * rv.double(), m * unb
        z = torch.zeros_like(mean)
        out.update(running_mean=a0 + a1, running_var=v0 + v1, unbiased=unb,
                   tol_running_mean=(1.0 - m) * (e_rm if e_rm is not None else z) + m * e_mean + 3.0 * U * (a0.abs() + a1.abs()),
                   tol_running_var=(1.0 - m) * (e_rv if e_rv is not None else z) + m * e_unb + 3.0 * U * (v0.abs() + v1.abs()))
    return out


def _z(x, scale, shift):
    """(z, e_z) in fp64 from the fp32 scale and shift"""
    xs = x.double() * scale.double()
    z = xs + shift.double()
    e_z = U * xs.abs() + U * z.abs()
    exact = (xs.float().double() == xs) & (z.float().double() == z)
    return z, torch.where(exact, torch.zeros_like(e_z), e_z)


def _first_max(x, z, e_z, S):
    """(arg int64 (G, C), zmax, e at the arg row, max_s e_z) of the groups of S rows; asserts that no group is contested"""
    R, C = z.shape
    G = R // S
    zv, ev, xv = z.view(G, S, C), e_z.view(G, S, C), x.float().view(G, S, C)
    zmax, emax = zv.amax(1), ev.amax(1)
    s_idx = torch.arange(S).view(1, S, 1)
    arg = torch.where(zv == zmax[:, None], s_idx, S).amin(1)
    x_arg = xv.gather(1, arg[:, None])
    contested = ((zmax[:, None] - zv) <= 2.0 * emax[:, None]) & (xv != x_arg) & (emax[:, None] > 0)
    n = int(contested.any(1).sum())
    assert n == 0, "%d contested groups (another x value within 2 max e_z of the maximum)" % n
    return arg, zmax, ev.gather(1, arg[:, None])[:, 0], emax


def apply(x, scale, shift, S=0, relu=True, pool=False):
    """fp64 y with tol_y and its fp32 part e_y; pooled: (R / S, C) and arg, uint8 when S <= 256"""
    z, e_z = _z(x, scale, shift)
    arg = None
    if pool:
        arg, z, _, e_z = _first_max(x, z, e_z, S)
    if relu:
        e_z = torch.where(z < -e_z, torch.zeros_like(e_z), e_z)
        z = z.clamp_min(0.0)
    if arg is not None and S <= 256:
        arg = arg.to(torch.uint8)
    return dict(y=z, e_y=e_z, tol_y=_bf16_tol(z, e_z), arg=arg)


def backward(dy, x, st, S=0, relu=True, pool=False):
    """fp64 dx (R, C), dgamma, dbeta with tol_dx (bf16), tol_dgamma, tol_dbeta (fp32; *_arg: for the table-reading reduce, where
    it exists) and e_dx, from st = the f32 (4, C) scale | shift | mean | rstd the kernel is given.  Pooled: dy is (R / S, C);
    arg, g (the routed gradient, (R, C)) are returned too.  undecided: the count of undecided ReLU masks"""
    R, C = x.shape
    sc, sh, mu, rs = (st[i].double() for i in range(4))
    xd, dyd = x.double(), dy.double()
    z, e_z = _z(x, st[0], st[1])
    xhat = (xd - mu) * rs
    e_xh = 2.0 * U * xhat.abs()
    arg = None
    if pool:
        G = R // S
        arg, zsel, esel, _ = _first_max(x, z, e_z, S)
        scat = lambda v: torch.zeros(G, S, C, dtype=torch.float64).scatter_(1, arg[:, None], v[:, None]).view(R, C)
        und = (zsel.abs() <= esel) & (esel > 0) if relu else torch.zeros_like(zsel, dtype=torch.bool)
        live = (zsel > 0) if relu else torch.ones_like(zsel, dtype=torch.bool)
        n_und, n_el = int(und.sum()), und.numel()
        g, dyfull, und = scat(dyd * live), scat(dyd), scat(und.double())
    else:
        und = ((z.abs() <= e_z) & (e_z > 0) if relu else torch.zeros_like(z, dtype=torch.bool))
        n_und, n_el = int(und.sum()), und.numel()
        g, dyfull, und = (dyd * (z > 0) if relu else dyd), dyd, und.double()
    assert n_und <= UNDECIDED_CAP * n_el, "%d of %d ReLU masks undecided" % (n_und, n_el)
    del z, e_z
    gx = g * xhat
    dbeta, dgamma = g.sum(0), gx.sum(0)
    gabs = g.abs() + dyfull.abs() * und
    gain_b, gain_g = (dyfull.abs() * und).sum(0), ((dyfull * xhat).abs() * und).sum(0)
    sum_g, sum_gx, sum_ge = gabs.sum(0), (gabs * xhat.abs()).sum(0), (gabs * e_xh).sum(0)
    out = dict(dbeta=dbeta, dgamma=dgamma, arg=arg, g=g, undecided=n_und)
    forms = [("", False)] + ([("_arg", True)] if pool and C <= 256 and S <= 256 else [])
    for sfx, table in forms:
        Du = (depth(R, C, S, pool, table, backward=True)[0] + 8) * U
        out["tol_dbeta" + sfx] = Du * sum_g + gain_b
        out["tol_dgamma" + sfx] = Du * sum_gx + sum_ge + gain_g
    mb, mg = dbeta / R, dgamma / R
    e_mb = out["tol_dbeta"] / R + 2.0 * U * mb.abs()
    e_mg = out["tol_dgamma"] / R + 2.0 * U * mg.abs()
    A = g.abs() + mb.abs() + (xhat * mg).abs()
    e_t = 3.0 * U * A + e_mb + xhat.abs() * e_mg + mg.abs() * e_xh
    dx = sc * (g - mb - xhat * mg)
    e_dx = sc.abs() * (e_t + U * A)
    out.update(dx=dx, e_dx=e_dx, tol_dx=_bf16_tol(dx, e_dx) + (sc * dyfull).abs() * und)
    return out


# ---- the whole-tensor norms of test_fused_batchnorm_relu_maxpool_point_major, restated ----------------------------------------------
OLD_NORMS = dict(y=6e-3, dx=2e-2, dgamma=1e-2, dbeta=1e-2, running_mean=1e-4, running_var=1e-4)


def old_norms_accept(kind, out, ref):
    """rel-L2 below 6e-3 for the output, 2e-2 for dx, 1e-2 for dgamma / dbeta, 1e-4 for the running statistics"""
    out, ref = out.float(), ref.float()
    rel = ((out - ref).norm() / (ref.norm() + 1e-12)).item()
    return bool(torch.isfinite(out).all()) and rel < OLD_NORMS[kind]


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------
def _chunk_sums(v, per, ph):
    """fp32 (n, W) -> (n_c, W): per partial, thread phase p adds the terms p, p + ph, ... of its chunk in order, then the ph
    phase sums are added in order (bn_stats_kernel, bn_bwd_reduce_kernel, bn_bwd_reduce_arg_kernel)"""
    n, W = v.shape
    n_c, n_t = _cdiv(n, per), _cdiv(per, ph)
    flat = torch.zeros(n_c * per, W, dtype=torch.float32)
    flat[:n] = v
    buf = torch.zeros(n_c, n_t * ph, W, dtype=torch.float32)
    buf[:, :per] = flat.view(n_c, per, W)
    buf = buf.view(n_c, n_t, ph, W)
    acc = torch.zeros(n_c, ph, W, dtype=torch.float32)
    for i in range(n_t):
        acc = acc + buf[:, i]
    out = torch.zeros(n_c, W, dtype=torch.float32)
    for p in range(ph):
        out = out + acc[:, p]
    return out


def _fold(part, phases):
    """the fold of the partials (n_c, W): fold_column (phases = 4: trip 32, the phases added as a tree) or bn_fold_kernel
    (phases = 16: trip 128, the phases added in order)"""
    n_c, W = part.shape
    s = []
    for ph in range(phases):
        t = [torch.zeros(W, dtype=torch.float32) for _ in range(8)]
        y = ph
        while y + phases * 7 < n_c:
            for u in range(8):
                t[u] = t[u] + part[y + phases * u]
            y += phases * 8
        while y < n_c:
            t[0] = t[0] + part[y]
            y += phases
        s.append(((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])))
    if phases == 4:
        return (s[0] + s[1]) + (s[2] + s[3])
    v = torch.zeros(W, dtype=torch.float32)
    for q in range(phases):
        v = v + s[q]
    return v


def emulate_stats(x, gamma, beta, eps, momentum, rm=None, rv=None, pivot_roll=0):
    """f32 (4, C) scale | shift | mean | rstd and the updated running_mean, running_var (or None), with the kernels' rounding
    points (products uncontracted).  pivot_roll: a planted defect -- channel c takes x[0, c + pivot_roll] for its pivot, in both
    kernels"""
    R, C = x.shape
    f = torch.float32
    xf = x.float()
    p = xf[0].roll(-pivot_roll) if pivot_roll else xf[0]
    t = xf - p
    part = _chunk_sums(torch.cat([t, t * t], 1), chunk_rows(R), 2048 // C)
    tot = _fold(part, 4)
    invR = torch.tensor(1.0, dtype=f) / torch.tensor(float(R), dtype=f)
    dmean = tot[:C] * invR
    mean = p + dmean
    var = (tot[C:] * invR - dmean * dmean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=f))
    sc = gamma.float() * rstd
    st = torch.stack([sc, beta.float() - mean * sc, mean, rstd])
    if rm is None:
        return st, None, None
    m, one = torch.tensor(momentum, dtype=f), torch.tensor(1.0, dtype=f)
    unb = var * (torch.tensor(float(R), dtype=f) / torch.tensor(float(R - 1), dtype=f)) if R > 1 else var
    return st, (one - m) * rm.float() + m * mean, (one - m) * rv.float() + m * unb


def _first_arg32(z, S):
    G, C = z.shape[0] // S, z.shape[1]
    zv = z.view(G, S, C)
    zmax = zv.amax(1)
    return torch.where(zv == zmax[:, None], torch.arange(S).view(1, S, 1), S).amin(1), zmax


def emulate_apply(x, scale, shift, S=0, relu=True, pool=False):
    """(y bf16, arg int64 or None)"""
    z = x.float() * scale.float() + shift.float()
    arg = None
    if pool:
        arg, z = _first_arg32(z, S)
    return _bf(z.clamp_min(0.0) if relu else z), arg


def emulate_backward(dy, x, st, S=0, relu=True, pool=False, table=None):
    """(dx bf16, dgamma, dbeta): the partial sums in chunk, phase and fold order; table: the arg-max table the table-reading
    reduce is handed (dx is the searching kernel's either way)"""
    R, C = x.shape
    sc, sh, mu, rs = (st[i].float() for i in range(4))
    xf, dyf = x.float(), dy.float()
    z = xf * sc + sh
    xhat = (xf - mu) * rs
    if pool:
        G = R // S
        arg, zmax = _first_arg32(z, S)
        idx = (table.long() if table is not None else arg)[:, None]
        xsel = xf.view(G, S, C).gather(1, idx)[:, 0]
        zsel = xsel * sc + sh
        gsel = torch.where(zsel > 0, dyf, torch.zeros_like(dyf)) if relu else dyf
        terms = torch.cat([gsel, gsel * ((xsel - mu) * rs)], 1)
        gk = torch.where(zmax > 0, dyf, torch.zeros_like(dyf)) if relu else dyf
        g = torch.zeros(G, S, C, dtype=torch.float32).scatter_(1, arg[:, None], gk[:, None]).view(R, C)
    else:
        g = torch.where(z > 0, dyf, torch.zeros_like(dyf)) if relu else dyf
        terms = torch.cat([g, g * xhat], 1)
    _, per, ph, _ = layout(R, C, S, pool, table is not None)
    dgb = _fold(_chunk_sums(terms, per, ph), 16)
    invR = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(R), dtype=torch.float32)
    mb, mg = dgb[:C] * invR, dgb[C:] * invR
    dx = sc * (g - mb - xhat * mg)
    return _bf(dx), dgb[C:], dgb[:C]


# ---- the cases of tests/test_bn_bound_gpu.py (the CPU module checks its caps and bookkeeping on the same list) --------------------
BIG_LO, BIG_HI = (1 << 20) - 64, (1 << 20) + 64      # either side of the chunk-size switch


def _st(R, C, eps=1e-5, m=0.1, run=True):
    return dict(R=R, C=C, eps=eps, m=m, run=run)


# every width at R = 300 (C >= 512: fewer than 256 / rps sweeps, C = 2048: rps = 1); C = 8 with 1, 1, 1, 1, 2, 5, 17, 34 and 130
# partials (both sides of fold_column's 4-phase tail and of its trip of 32; 130 also crosses bn_fold_kernel's trip of 128 in
# the backward cases); the chunk-size switch
STATS_CASES = ([_st(300, C, eps=(1e-5, 1e-3)[i % 2], m=(0.1, 0.01)[(i // 2) % 2], run=i % 3 != 2) for i, C in enumerate(WIDTHS)]
               + [_st(R, 8, eps=(1e-3, 1e-5)[i % 2], m=(0.01, 0.1)[i % 2], run=i % 4 != 3)
                  for i, R in enumerate((1, 3, 255, 256, 257, 1025, 4097, 8453, 33041))]
               + [_st(1500, 64), _st(BIG_LO, 8, m=0.01), _st(BIG_HI, 8, eps=1e-3)])


def _ap(R, C, S=0, relu=True, arg=False):
    return dict(R=R, C=C, S=S, relu=relu, pool=S > 0, arg=arg)


# group counts of 1, 255 and counts that are no multiple of the 256 / tpr groups a workgroup takes (tpr = C / 8 threads per row)
APPLY_CASES = [
    _ap(300, 8), _ap(257, 64, relu=False), _ap(33, 256), _ap(5, 2048, relu=False),
    _ap(37, 8, 1, arg=True), _ap(2 * 255, 64, 2, relu=False, arg=True), _ap(16 * 529, 64, 16, arg=True),
    _ap(32 * 33, 256, 32, relu=False, arg=True), _ap(64, 8, 64, arg=True), _ap(256 * 5, 8, 256, relu=False, arg=True),
    _ap(16 * 3, 2048, 16, arg=True), _ap(512 * 3, 8, 512), _ap(1024 * 2, 64, 1024, relu=False), _ap(8192 * 2, 8, 8192),
]


def _bw(R, C, S=0, relu=True):
    return dict(R=R, C=C, S=S, relu=relu, pool=S > 0)


# unpooled R of 1, 257, 8453; pooled: G = 5 < rps, G = 16 * 33 + 1 (gpc = 16), S = 512 (gpc = 1), S = 8192 (one group per
# partial, S > 4096), gpc = 4 at C = 2048 with G = 9; the two R ~ 2^20 shapes pooled over 64 (gpc = 4 | 16, 4096 | 1025 partials)
BWD_CASES = [
    _bw(1, 8), _bw(257, 64, relu=False), _bw(8453, 8), _bw(257, 512), _bw(1, 2048, relu=False), _bw(257, 2048),
    _bw(8453, 64, relu=False), _bw(257, 8, relu=False), _bw(257, 64), _bw(257, 512, relu=False),
    _bw(16 * 5, 8, 16), _bw(16 * 529, 64, 16), _bw(16 * 529, 64, 16, relu=False), _bw(512 * 3, 512, 512),
    _bw(8192 * 2, 8, 8192, relu=False), _bw(64 * 9, 2048, 64), _bw(512 * 3, 512, 512, relu=False),
    _bw(64 * 9, 2048, 64, relu=False), _bw(BIG_LO, 8, 64), _bw(BIG_HI, 8, 64, relu=False),
]

# the table-reading reduce: G < gps, G = gpc k + 1, one group per partial
TABLE_CASES = [
    _bw(16 * 529, 64, 16), _bw(64 * 5, 8, 64, relu=False), _bw(256 * 3, 256, 256), _bw(64 * 9, 256, 64, relu=False),
    _bw(16 * 33, 8, 16), _bw(16 * 529, 64, 16, relu=False),
]


def case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items() if k != "pool")
