"""Reference, bounds, fp32 emulation and inputs of the kernels of csrc/mcan.hip (include/bqhip_mcan.h): MCAN's residual LayerNorm
forward / backward and AttFlat's masked softmax pooling forward / backward, for tests/test_mcan_rows_cpu.py and
tests/test_mcan_rows_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  fp64 from the fp32 operands the kernels see.
    LayerNorm forward    z = x + s, mean = sum_j z / H, c = z - mean, sigma = sqrt(sum_j c^2 / (H - 1)), r = 1 / (sigma + eps),
                         q = c r, y = a2 q + b2                                  (eps: the fp32 value the kernel is given)
    LayerNorm backward   mean and sigma are GIVEN fp32 values (the kernel reads them; exact in the reference too):
                         g = dy a2, s1 = mean_j g, s2 = sum_j g c, k = r^2 / ((H - 1) sigma), dz = r (g - s1) - k s2 c,
                         da2 = sum_rows dy q, db2 = sum_rows dy
    pool forward         l = hide ? -1e9 : logit (fp32(-1e9) is exactly -1e9), p = softmax_n(l),
                         out[b, g H + h] = sum_n p[b, n, g] x[b, n, h]
    pool backward        p GIVEN (fp32): dx = sum_g p dout, da = sum_h x dout, t = sum_n p da, dl = hide ? 0 : p (da - t)

BOUNDS, per element.  u = 2^-24, Hu = (H + 8) u, Nu = (N + 8) u, Mu = (M + 8) u: a sum of K fp32 terms in ANY order errs by at
most (K - 1) u sum|terms| to first order, and the 8 covers the elementwise roundings around each sum.  mean_j / rms_j / max_j run
over the row.

  LayerNorm forward
    z     one rounding:  e_z = u |z| (0 without s);  az = |x| + |s| >= |z| is what the sum's roundings are relative to
    mean  e_m = Hu mean_j az
    c     e_c = e_z + e_m + u |c|
    ss = sum_j c^2.  An error dm of the mean enters only as dm^2 (sum_j c_j = 0), an error dz_j of z as 2 c_j dz_j
          (Cauchy-Schwarz over the row), the H-term sum, the products and the rounding of c as (H + 2) u:
          rel_ss = (H + 4) u + 2 sqrt(H / (H - 1)) rms_j(e_z) / sigma + (H / (H - 1)) ((e_m + max_j e_z) / sigma)^2
    sigma division by H - 1 and sqrtf:   rel_sigma = rel_ss / 2 + 2 u
    r     the sum sigma + eps, the division:   rel_r = rel_sigma sigma / (sigma + eps) + 2 u
    q     e_q = r e_c + |q| (rel_r + u)
    y     e_y = |a2| e_q + u |a2 q| + u |y|
    mean is held to e_m, sigma to sigma rel_sigma.
    A constant row has sigma = 0: every relative term above is x / 0.  There the kernel's result is exact instead (c = 0, q = 0,
    y = b2 bit for bit) and the tests require that; the row is left out of the bound comparison and of every backward case.

  LayerNorm backward (mean, sigma given)
    c     e_c = e_z + u |c|
    s1    e_s1 = Hu mean_j |g|                        s2    e_s2 = Hu sum_j |g c| + sum_j |g| e_c
    dz    e_dz = r (3 u (|g| + |s1|) + e_s1) + k (|c| e_s2 + |s2| e_c + 8 u |s2 c|) + u |dz|
                 + 2 u (r |g - s1| + 2 k |s2 c|)
          The last line is an ADDED term.  The 3 u and the 8 u count the operations that combine g, s1, s2, c with r and k --
          g's product, the subtraction, the product with r; r r, (H - 1) sigma, the division, k s2, its product with c -- as if r
          itself were exact.  The kernel forms r = 1 / (sigma + eps) in fp32 from the given sigma: two roundings, 2 u relative,
          which reach the first product once and k = r^2 / ... twice.
    da2   Mu sum_rows |dy q| + sum_rows |dy| (r e_c + 3 u |q|)      (q = c r: e_c, r's two roundings, the product)
    db2   Mu sum_rows |dy|

  pool forward
    p     the rounding of l - max is an absolute error u |l - max| of the exponent, expf is 1 ulp, the N positive terms, the
          division:   rel_p[n] = (|l_n - max| + N + 16) u,   tol_p = p rel_p
          (a hidden key next to a visible one has p = 0 exactly, in fp32 and in the fp64 reference alike: exp(-1e9)
          underflows in both, and the tolerance there is 0)
    out   tol_out[h] = sum_n |p_n x_nh| (rel_p[n] + Nu)

  pool backward (p given)
    dx    (G + 2) u sum_g |p dout|
    da    e_da = Hu sum_h |x dout|
    t     e_t = Nu sum_n |p da| + sum_n p e_da
    dl    p (e_da + e_t + u (|da| + |t|)) + u |dl|;  exactly 0, tolerance 0, at hidden positions

EMULATION.  The same arithmetic in fp32 tensors on the host with the kernels' rounding points and order of additions: a lane owns
columns i 64 + lane and adds its values for ascending i, the 64 lane sums are folded by halves (the xor butterfly 32, 16, .. 1);
the LayerNorm backward strides rows over min(ceil(M / 4), 256) workgroups of 4 waves, folds the waves as (w0 + w1) + (w2 + w3)
and adds the workgroups' partials as mcan_ln_fold_kernel does (32 interleaved chains, then a tree); the pooled sum runs over ascending n.  Only expf / sqrtf may differ from
the device in the last bit.  The emulations take `defect`, which plants one named error for tests/test_mcan_rows_cpu.py.
"""
import functools
import zlib

import torch

from ln_ref import excess  # noqa: F401  (the per-element comparison, shared)

U = 2.0 ** -24
EPS = 1e-6                  # mcan_module.LayerNorm's default
FILL = -1e9
BWD_CAP = 256               # include/bqhip_mcan.h: BQ_MCAN_LN_BWD_CAP
CONST_ROW = 3

LN_SHAPES = [(M, H) for M in (1, 5, 67) for H in (64, 256, 1024)]
POOL_SHAPES = [(3, N, G, H) for N in (1, 37, 256) for G in (1, 2) for H in (64, 256)]
MASKS = ("none", "mixed")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def eps32(eps=EPS):
    return float(torch.tensor(eps, dtype=torch.float32))


# ---- the compositions of bridgeqa_amd/mcan_module.py as they stood before the fused route: what "unchanged" means -------------------
def composition_layernorm(m, x):
    centred = x - x.mean(-1, keepdim=True)
    n = x.shape[-1]
    std = centred.pow(2).sum(-1, keepdim=True).div(max(n - 1, 1)).sqrt()
    return m.a_2 * centred / (std + m.eps) + m.b_2


def composition_attflat_tail(att, x, x_mask, glimpses):
    if x_mask is not None:
        att = att.masked_fill(x_mask.squeeze(1).squeeze(1).unsqueeze(2), -1e9)
    att = torch.softmax(att, dim=1)
    return torch.cat([torch.sum(att[:, :, i:i + 1] * x, dim=1) for i in range(glimpses)], dim=1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_inputs(M, H):
    """dict of x, s, dy (f32 (M, H)), a2, b2 (f32 (H,)), seeded by the shape.  x ~ 2 N(0, 1), s ~ 3 N(0, 1) + 0.5; row 1 has mean
    40 and unit spread; row 2 is x and s scaled by 1e-3 with zero mean (sigma within a few thousand eps: the one row on which a
    misplaced eps shows); row 3 is constant (x = 1.5, s = 0.5).  a2 in [0.5, 1.5] with a2[5] = 0 and a2[H - 3] = -0.75.
    Shared between tests: do not write to the tensors."""
    g = torch.Generator().manual_seed(_seed("mcan_ln", M, H))
    x = torch.randn(M, H, generator=g) * 2.0
    s = torch.randn(M, H, generator=g) * 3.0 + 0.5
    if M > 1:
        x[1] = torch.randn(H, generator=g) + 40.0
        s[1] = torch.randn(H, generator=g) * 0.25
    if M > 2:
        x[2] = torch.randn(H, generator=g) * 2e-3
        s[2] = torch.randn(H, generator=g) * 3e-3
    if M > CONST_ROW:
        x[CONST_ROW] = 1.5
        s[CONST_ROW] = 0.5
    dy = torch.randn(M, H, generator=g)
    a2 = torch.rand(H, generator=g) + 0.5
    a2[5], a2[H - 3] = 0.0, -0.75
    b2 = torch.randn(H, generator=g) * 0.1
    return dict(x=x, s=s, dy=dy, a2=a2, b2=b2)


def regular_rows(M):
    """bool (M,): the rows held to the bound (all but the constant one)"""
    keep = torch.ones(M, dtype=torch.bool)
    if M > CONST_ROW:
        keep[CONST_ROW] = False
    return keep


@functools.lru_cache(maxsize=None)
def ln_bwd_inputs(M, H, with_s=True):
    """the backward's operands: ln_inputs(M, H) WITHOUT the constant row (its gradient is NaN by construction), and mean / sigma
    of the fp64 rows rounded once to fp32 -- what a backward test hands to the kernel AND to the reference"""
    d = ln_inputs(M, H)
    keep = regular_rows(M)
    x, s, dy = d["x"][keep].contiguous(), d["s"][keep].contiguous(), d["dy"][keep].contiguous()
    if not with_s:
        s = None
    z = x.double() + (s.double() if s is not None else 0.0)
    mean = z.mean(1, keepdim=True)
    sigma = ((z - mean).square().sum(1) / (H - 1)).sqrt()
    return dict(x=x, s=s, dy=dy, a2=d["a2"], mean=mean[:, 0].float(), sigma=sigma.float())


def pool_hide(B, N, kind):
    """bool (B, N), True = hidden, or None.  "mixed": sample 0 has its tail hidden (the last third), sample 1 is hidden
    completely, sample 2 shows the single key N // 2"""
    if kind == "none":
        return None
    assert kind == "mixed" and B >= 3
    hide = torch.zeros(B, N, dtype=torch.bool)
    hide[0, N - N // 3:] = True
    hide[1] = True
    hide[2] = True
    hide[2, N // 2] = False
    return hide


@functools.lru_cache(maxsize=None)
def pool_inputs(B, N, G, H):
    """dict of x (B, N, H) ~ N(0, 1), logits (B, N, G) ~ 3 N(0, 1), dout (B, G H) ~ N(0, 1), seeded by the shape; read-only"""
    g = torch.Generator().manual_seed(_seed("mcan_pool", B, N, G, H))
    return dict(x=torch.randn(B, N, H, generator=g), logits=torch.randn(B, N, G, generator=g) * 3.0,
                dout=torch.randn(B, G * H, generator=g))


def pool_p32(logits, hide):
    """the reference's p rounded once to fp32: what a pool-backward test hands to the kernel AND to the reference"""
    return pool_forward(torch.zeros(logits.shape[0], logits.shape[1], 64), logits, hide)["p"].float()


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def _z(x, s):
    xd = x.double()
    if s is None:
        return xd, torch.zeros_like(xd), xd.abs()
    sd = s.double()
    z = xd + sd
    return z, U * z.abs(), xd.abs() + sd.abs()


def ln_forward(x, s, a2, b2, eps=EPS):
    """fp64 mean, sigma, y and tol_mean, tol_sigma, tol_y (inf / NaN on a constant row: leave it out)"""
    H = x.shape[1]
    Hu = (H + 8) * U
    eps = eps32(eps)
    a, b = a2.double(), b2.double()
    z, e_z, az = _z(x, s)
    mean = z.mean(1, keepdim=True)
    c = z - mean
    sigma = (c.square().sum(1, keepdim=True) / (H - 1)).sqrt()
    r = 1.0 / (sigma + eps)
    q = c * r
    y = a * q + b
    e_m = Hu * az.mean(1, keepdim=True)
    e_c = e_z + e_m + U * c.abs()
    ratio = H / (H - 1.0)
    rel_ss = ((H + 4) * U + 2.0 * ratio ** 0.5 * e_z.square().mean(1, keepdim=True).sqrt() / sigma
              + ratio * ((e_m + e_z.amax(1, keepdim=True)) / sigma).square())
    rel_sigma = rel_ss / 2.0 + 2.0 * U
    rel_r = rel_sigma * sigma / (sigma + eps) + 2.0 * U
    e_q = r * e_c + q.abs() * (rel_r + U)
    e_y = a.abs() * e_q + U * (a * q).abs() + U * y.abs()
    return dict(mean=mean[:, 0], sigma=sigma[:, 0], y=y, tol_mean=e_m[:, 0], tol_sigma=(sigma * rel_sigma)[:, 0], tol_y=e_y)


def ln_backward(dy, x, s, a2, mean, sigma, eps=EPS):
    """fp64 dz, da2, db2 with tol_dz, tol_da2, tol_db2.  mean, sigma: the fp32 tensors the kernel is given."""
    M, H = x.shape
    Hu, Mu = (H + 8) * U, (M + 8) * U
    eps = eps32(eps)
    a, d = a2.double(), dy.double()
    z, e_z, _ = _z(x, s)
    m, sg = mean.double()[:, None], sigma.double()[:, None]
    c = z - m
    e_c = e_z + U * c.abs()
    r = 1.0 / (sg + eps)
    k = r * r / ((H - 1) * sg)
    g = d * a
    s1 = g.mean(1, keepdim=True)
    s2 = (g * c).sum(1, keepdim=True)
    e_s1 = Hu * g.abs().mean(1, keepdim=True)
    e_s2 = Hu * (g * c).abs().sum(1, keepdim=True) + (g.abs() * e_c).sum(1, keepdim=True)
    dz = r * (g - s1) - k * s2 * c
    e_dz = (r * (3.0 * U * (g.abs() + s1.abs()) + e_s1) + k * (c.abs() * e_s2 + s2.abs() * e_c + 8.0 * U * (s2 * c).abs())
            + U * dz.abs() + 2.0 * U * (r * (g - s1).abs() + 2.0 * k * (s2 * c).abs()))
    q = c * r
    return dict(dz=dz, da2=(d * q).sum(0), db2=d.sum(0), tol_dz=e_dz,
                tol_da2=Mu * (d * q).abs().sum(0) + (d.abs() * (r * e_c + 3.0 * U * q.abs())).sum(0),
                tol_db2=Mu * d.abs().sum(0))


def _filled(logits, hide, fill=FILL):
    l = logits.double()
    return l if hide is None else l.masked_fill(hide[:, :, None], fill)


def pool_forward(x, logits, hide):
    """fp64 p (B, N, G), out (B, G H) with tol_p, tol_out"""
    B, N, G = logits.shape
    Nu = (N + 8) * U
    l = _filled(logits, hide)
    d = l - l.amax(1, keepdim=True)
    p = torch.softmax(l, dim=1)
    rel_p = (d.abs() + N + 16) * U
    xd = x.double()
    out = torch.einsum("bng,bnh->bgh", p, xd).reshape(B, -1)
    tol_out = torch.einsum("bng,bnh->bgh", p * (rel_p + Nu), xd.abs()).reshape(B, -1)
    return dict(p=p, out=out, tol_p=p * rel_p, tol_out=tol_out)


def pool_backward(dout, x, p, hide):
    """fp64 dx (B, N, H), dlogits (B, N, G) with tol_dx, tol_dl.  p: the fp32 tensor the kernel is given."""
    B, N, H = x.shape
    G = p.shape[2]
    Hu, Nu = (H + 8) * U, (N + 8) * U
    pd, xd, dd = p.double(), x.double(), dout.double().view(B, G, H)
    dx = torch.einsum("bng,bgh->bnh", pd, dd)
    tol_dx = (G + 2) * U * torch.einsum("bng,bgh->bnh", pd.abs(), dd.abs())
    da = torch.einsum("bnh,bgh->bng", xd, dd)
    e_da = Hu * torch.einsum("bnh,bgh->bng", xd.abs(), dd.abs())
    t = (pd * da).sum(1, keepdim=True)
    e_t = Nu * (pd * da).abs().sum(1, keepdim=True) + (pd * e_da).sum(1, keepdim=True)
    dl = pd * (da - t)
    tol_dl = pd * (e_da + e_t + U * (da.abs() + t.abs())) + U * dl.abs()
    if hide is not None:
        dl = dl.masked_fill(hide[:, :, None], 0.0)
        tol_dl = tol_dl.masked_fill(hide[:, :, None], 0.0)
    return dict(dx=dx, dl=dl, tol_dx=tol_dx, tol_dl=tol_dl)


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------
def _fold64(s):
    """(..., 64) lane values -> (..., 1): the xor butterfly 32, 16, .. 1 adds halves"""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s


def _wave_sum(v):
    """sums over the last axis (a multiple of 64) as one wave forms them: lane l adds its values i 64 + l for ascending i"""
    t = v.reshape(v.shape[:-1] + (v.shape[-1] // 64, 64))
    s = torch.zeros(v.shape[:-1] + (64,), dtype=torch.float32)
    for i in range(t.shape[-2]):
        s = s + t[..., i, :]
    return _fold64(s)


def _pad64(v):
    """zero-pad the last axis to a multiple of 64 (a lane without an element adds nothing)"""
    n = v.shape[-1]
    return torch.nn.functional.pad(v, (0, -n % 64))


def _round16(c):
    return c.to(torch.bfloat16).float()


def emulate_ln_forward(x, s, a2, b2, eps=EPS, defect=None):
    """y, mean, sigma in fp32 with the kernel's rounding points.  defect: "divisor_H", "eps_in_sqrt", "c_16bit" """
    H = x.shape[1]
    e = torch.tensor(eps, dtype=torch.float32)
    z = x + s if s is not None else x.clone()
    mean = _wave_sum(z) / float(H)
    c = z - mean
    if defect == "c_16bit":
        c = _round16(c)
    var = _wave_sum(c * c) / float(H if defect == "divisor_H" else H - 1)
    if defect == "eps_in_sqrt":
        sigma = torch.sqrt(var)
        r = 1.0 / torch.sqrt(var + e)
    else:
        sigma = torch.sqrt(var)
        r = 1.0 / (sigma + e)
    y = a2 * (c * r) + b2
    return y, mean[:, 0], sigma[:, 0]


def emulate_ln_backward(dy, x, s, a2, mean, sigma, eps=EPS, defect=None):
    """dz (M, H), da2, db2 (H) in fp32: the kernel's roundings, row-to-wave assignment and fold order.  defect: "c_16bit" """
    M, H = x.shape
    e = torch.tensor(eps, dtype=torch.float32)
    z = x + s if s is not None else x.clone()
    m, sg = mean[:, None], sigma[:, None]
    r = 1.0 / (sg + e)
    k = (r * r) / (float(H - 1) * sg)
    c = z - m
    if defect == "c_16bit":
        c = _round16(c)
    g = dy * a2
    s1 = _wave_sum(g) / float(H)
    ks2 = k * _wave_sum(g * c)
    dz = r * (g - s1) - ks2 * c
    blocks = min((M + 3) // 4, BWD_CAP)
    slots = blocks * 4
    aa = torch.zeros(slots, H, dtype=torch.float32)
    ab = torch.zeros(slots, H, dtype=torch.float32)
    dq = dy * (c * r)
    for r0 in range(0, M, slots):
        n = min(slots, M - r0)
        aa[:n] = aa[:n] + dq[r0:r0 + n]
        ab[:n] = ab[:n] + dy[r0:r0 + n]
    aa, ab = aa.view(blocks, 4, H), ab.view(blocks, 4, H)
    pa = (aa[:, 0] + aa[:, 1]) + (aa[:, 2] + aa[:, 3])
    pb = (ab[:, 0] + ab[:, 1]) + (ab[:, 2] + ab[:, 3])
    return dz, _fold_slab(pa), _fold_slab(pb)


def _fold_slab(part):
    """mcan_ln_fold_kernel: partial k goes to accumulator (k // 4) % 8 of row phase k % 4, in ascending k; then two trees"""
    t = torch.zeros(4, 8, part.shape[1], dtype=torch.float32)
    for k in range(part.shape[0]):
        t[k % 4, (k // 4) % 8] = t[k % 4, (k // 4) % 8] + part[k]
    s = ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7]))
    return (s[0] + s[1]) + (s[2] + s[3])


def emulate_pool_forward(x, logits, hide, defect=None):
    """out (B, G H), p (B, N, G) in fp32.  defect: "fill_inf" """
    B, N, G = logits.shape
    fill = float("-inf") if defect == "fill_inf" else FILL
    l = logits if hide is None else logits.masked_fill(hide[:, :, None], fill)
    lt = l.transpose(1, 2)                                   # (B, G, N)
    e = torch.exp(lt - lt.amax(2, keepdim=True))
    p = (e / _wave_sum(_pad64(e))).transpose(1, 2).contiguous()
    acc = torch.zeros(B, G, x.shape[2], dtype=torch.float32)
    for n in range(N):
        acc = acc + p[:, n, :, None] * x[:, n, None, :]
    return acc.reshape(B, -1), p


def emulate_pool_backward(dout, x, p, hide, defect=None):
    """dx (B, N, H), dlogits (B, N, G) in fp32.  defect: "no_zero" (hidden dlogits not zeroed)"""
    B, N, H = x.shape
    G = p.shape[2]
    d = dout.view(B, G, H)
    dx = p[:, :, 0, None] * d[:, None, 0]
    for g in range(1, G):
        dx = dx + p[:, :, g, None] * d[:, None, g]
    da = _wave_sum(x[:, :, None, :] * d[:, None, :, :])[..., 0]                 # (B, N, G)
    t = _wave_sum(_pad64((p * da).transpose(1, 2)))                              # (B, G, 1)
    dl = p * (da - t.transpose(1, 2))
    if hide is not None and defect != "no_zero":
        dl = dl.masked_fill(hide[:, :, None], 0.0)
    return dx, dl
