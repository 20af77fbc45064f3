"""Reference, bound, inputs, emulation and planted defects of the LM head + label-smoothed cross entropy: the EPI_BIAS_CE
epilogue of gemm256_kernel (csrc/gemm.hip), lmhead_ce_combine_kernel and lmhead_ce_dlogits_kernel (csrc/lmhead.hip), for
tests/test_lmhead_bound_cpu.py and tests/test_lmhead_bound_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  fp64 from the bf16 h (R, D), the bf16 w (V, D) and the fp32 bias the kernel sees; the smoothing eps is the C float
the launcher passes.  Per row over v < V:
    z = h w^T + bias,   p = softmax(z),   L = logsumexp(z),   zbar = mean_v z
    loss = (1 - eps)(L - z_t) + eps (L - zbar)   for a target t >= 0,   0 for an ignored row
    dlogits = g (exp(x - l) - eps / V - (1 - eps)[v = t])   at the STORED bf16 logits x, the fp32 lse l and the fp32 g as given

BOUND.  u = 2^-24.
  z      e_z = 2 D u (|h||w|^T) + u |z|        (gemm_ref.bound's fp32 line with the bias add);   E = max_v e_z
  stored logits (R, Vp) bf16: gemm_ref.bound(w, h, bias, EPI_BIAS) for v < V; columns V .. Vp-1 are 0 exactly (the DMA reads
         zeros past the vocabulary matrix and the padded bias is 0 there)
  lse    tol_L = e^{2E} sum_v p_v e_z,v + rho_s + 2^-20 max(1, |L|) + u (|L| + |z_max|)
         logsumexp is 1-Lipschitz and its gradient is a softmax at an intermediate point, <= p e^{2E}; rho_s is the relative
         error of the kernel's sum of exponentials at its OWN fp32 logits:
             rho_s = 4 u sum_v p_v |z_v - z_max| + (V + 8 + 2 S) u + (1 + S) 2^-22
         every exponent (z - m) log2e takes three roundings, and the chain of rescales of a term telescopes to
         exp(m_local - m_final) with exponent errors that add up to 3 u |m_local - z_max| with the sign of the term's own (the
         fourth u: log2e itself is a rounded constant); the fp32 sum of V terms in any order errs by (V + 8) u; S = 2 (the
         xor-16 / xor-32 merges of the epilogue) + ceil(nrec / 64) (the combine's serial trips) + 6 (its xor shuffles) merge
         steps of two roundings and one v_exp_f32 (2^-22, the constant of tests/attn_ref.py) each, nrec = 2 ceil(Vp / 256);
         2^-20 max(1, |lse|) is v_log_f32 (attn_ref.py again) and the last term the rounding of m + log s.
  loss   tol = tol_L + (1 - eps) e_z,t + eps e_zbar + 4 u [(1 - eps)(|L| + |z_t|) + eps (|L| + |zbar|)]
         e_zbar = (sum_v e_z,v + (V + 8) u sum_v |z_v|) / V;   an ignored row's loss is 0 exactly
  dlogits  with phat = exp(x - l):  e_d = |g| [phat (3 u |x - l| + 2^-22) + 4 u (phat + eps / V + [v = t])] + (|g| + 2) 2^-126
         tol = 2^-8 (|d| + e_d) + e_d;   ignored rows and columns >= V are 0 exactly
         The last term of e_d is an amendment to the issue's bound: it has no term for underflow.  With eps = 0 a non-target
         element is g exp(x - l), and on the row whose logits span +-60, x - l reaches -120: exp(-120) = 8e-53 is below the
         smallest fp32 subnormal (1.4e-45), so fp32 arithmetic returns 0 -- exactly right to any relative precision that
         matters, and outside 2^-8 |d|.  Three places can lose up to 2^-126 absolutely (the smallest normal fp32 / bf16 number;
         below it a result is flushed or rounded on a fixed grid): the exponential (times |g|), the product with g, and the
         bf16 store.  1e-38 changes nothing for any element a defect can reach.

The emulation (emulate_forward / emulate_dlogits) restates the kernels' rounding points in fp32 torch, with the planted defects
of the CPU suite as switches.
"""
import functools
import math
import zlib

import torch

import gemm_ref as G

U = 2.0 ** -24
B8 = 2.0 ** -8
EXP_ERR = 2.0 ** -22      # v_exp_f32, relative (tests/attn_ref.py)
LOG_ERR = 2.0 ** -20      # v_log_f32, absolute at |lse| <= 1, relative above (tests/attn_ref.py)
TINY = 2.0 ** -126        # the smallest normal fp32 / bf16 number
LOG2E = 1.4426950408889634
IGNORE = -100

# (R, D, V): the smallest shapes at which each path exists
#   5, 64, 100    Vp = 128: the second half tile has no valid entry (-inf records reach the shuffle and the combine); R < 16
#   18, 256, 200  56 padding columns
#   70, 64, 256   no padding; crosses a wave's 64 rows
#   257, 64, 130  two row tiles with a one-row tail; two valid entries in half tile 1; Ni = 192 is a ragged i tile
#   3, 64, 8200   nrec = 66: the combine's second trip, ragged
SMALL_SHAPES = [(5, 64, 100), (18, 256, 200), (70, 64, 256), (257, 64, 130), (3, 64, 8200)]
SHIFT_SHAPE = (18, 64, 200)   # with the whole bias shifted by +90 and by -90: without the max subtraction e^90 overflows fp32
SHIFTS = (90.0, -90.0)        # and the terms e^-90 are below its normal range; the bound grows by u 90 only
PRODUCTION = (160, 768, 30524)
CASES = [s + (0.0,) for s in SMALL_SHAPES] + [SHIFT_SHAPE + (s,) for s in SHIFTS]   # (R, D, V, bias shift)
SMOOTHINGS = (0.1, 0.0, 0.3)


def padded(V):
    """Vp of fusion_ops._LMHeadCE: the vocabulary rounded up to 64"""
    return (V + 63) // 64 * 64


def n_records(V):
    """records per row: two half tiles per 256-wide vocabulary tile of the padded width"""
    return 2 * ((padded(V) + 255) // 256)


def f32(x):
    """the C float nearest to the Python float x, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=16)
def inputs(R, D, V, shift=0.0):
    """dict of h bf16 (R, D) ~ N(0, 1), w bf16 (V, D) ~ 0.1 N(0, 1), bias f32 (V,) ~ 0.5 N(0, 1) + shift, bias_pad f32 (Vp,),
    tgt int32 (R,), g f32 (R,) in [0.5, 1.5] (non-zero on ignored rows too), seeded by the shape.  Row 1 is h x 24 (a logit
    range of about +-60).  The targets of the first valid rows run through V-1, 0, 127, 128, 255, 256 (where < V) and the row's
    own argmax; row R // 2 (short shapes) or the row after those is ignored, as is a tenth of the rest; the last row -- the
    one-row tail of a ragged row tile -- is valid.  Shared between tests: do not write to the tensors."""
    gen = torch.Generator().manual_seed(_seed("lmhead", R, D, V, shift))
    h = torch.randn(R, D, generator=gen)
    if R > 1:
        h[1] *= 24.0
    h = h.to(torch.bfloat16)
    w = (torch.randn(V, D, generator=gen) * 0.1).to(torch.bfloat16)
    bias = torch.randn(V, generator=gen) * 0.5 + shift
    tgt = torch.randint(0, V, (R,), generator=gen).to(torch.int32)
    tgt[torch.rand(R, generator=gen) < 0.1] = IGNORE
    z = h.double() @ w.double().t() + bias.double()
    edges = [t for t in (V - 1, 0, 127, 128, 255, 256) if t < V] + ["argmax"]
    ign = R // 2 if R <= len(edges) + 1 else len(edges)
    rows = [r for r in range(R) if r != ign]
    for r, t in zip(rows, edges):
        tgt[r] = int(z[r].argmax()) if t == "argmax" else t
    tgt[ign] = IGNORE
    if tgt[R - 1] < 0:
        tgt[R - 1] = V // 2
    bias_pad = torch.zeros(padded(V), dtype=torch.float32)
    bias_pad[:V] = bias
    g = torch.rand(R, generator=gen) + 0.5
    return dict(h=h, w=w, bias=bias, bias_pad=bias_pad, tgt=tgt, g=g)


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def forward(h, w, bias):
    """the smoothing-independent part: fp64 z, p, L, zbar, z_max (rows), e_z, the stored-logits reference and tolerance
    (R, V), tol_L (R,) and the sums the loss bound needs.  bias: f32 (V,) or None"""
    D, V = h.shape[1], w.shape[0]
    z, tol_x = G.bound(w, h, bias, epi=G.EPI_BIAS)
    e_z = 2.0 * D * U * (h.double().abs() @ w.double().abs().t()) + U * z.abs()
    E = e_z.amax(1)
    L = torch.logsumexp(z, 1)
    p = torch.exp(z - L[:, None])
    zmax = z.amax(1)
    S = 2 + (n_records(V) + 63) // 64 + 6
    rho_s = 4.0 * U * (p * (z - zmax[:, None]).abs()).sum(1) + (V + 8 + 2 * S) * U + (1 + S) * EXP_ERR
    tol_L = torch.exp(2.0 * E) * (p * e_z).sum(1) + rho_s + LOG_ERR * L.abs().clamp(min=1.0) + U * (L.abs() + zmax.abs())
    zbar = z.mean(1)
    e_zbar = (e_z.sum(1) + (V + 8) * U * z.abs().sum(1)) / V
    return dict(z=z, tol_x=tol_x, e_z=e_z, p=p, L=L, zbar=zbar, zmax=zmax, tol_L=tol_L, e_zbar=e_zbar)


@functools.lru_cache(maxsize=8)
def forward_of(R, D, V, shift=0.0):
    """forward() at inputs(R, D, V, shift), computed once.  Do not write to the tensors."""
    d = inputs(R, D, V, shift)
    return forward(d["h"], d["w"], d["bias"])


def loss(f, tgt, smoothing):
    """(loss, tol, valid) of the rows, fp64 (R,): f = forward(...); ignored rows have loss 0 and tolerance 0"""
    eps = f32(smoothing)
    valid = tgt >= 0
    t = tgt.long().clamp(min=0)[:, None]
    zt = f["z"].gather(1, t)[:, 0]
    e_zt = f["e_z"].gather(1, t)[:, 0]
    L, zbar = f["L"], f["zbar"]
    r = (1.0 - eps) * (L - zt) + eps * (L - zbar)
    tol = (f["tol_L"] + (1.0 - eps) * e_zt + eps * f["e_zbar"]
           + 4.0 * U * ((1.0 - eps) * (L.abs() + zt.abs()) + eps * (L.abs() + zbar.abs())))
    zero = torch.zeros_like(r)
    return torch.where(valid, r, zero), torch.where(valid, tol, zero), valid


def dlogits(x, l, g, tgt, V, smoothing):
    """(d, tol, e_d) fp64 (R, Vp) at the stored bf16 logits x (R, Vp), the fp32 lse l and the fp32 g as given; ignored rows and
    columns >= V have d = 0 and tolerance 0"""
    eps = f32(smoothing)
    R, Vp = x.shape
    xd, ld, gd = x.double(), l.double()[:, None], g.double()[:, None]
    cols = torch.arange(Vp)[None, :]
    hot = (cols == tgt.long()[:, None]).double()
    live = (tgt >= 0)[:, None] & (cols < V)
    ph = torch.exp(xd - ld)
    d = gd * (ph - eps / V - (1.0 - eps) * hot)
    e_d = gd.abs() * (ph * (3.0 * U * (xd - ld).abs() + EXP_ERR) + 4.0 * U * (ph + eps / V + hot)) + (gd.abs() + 2.0) * TINY
    tol = B8 * (d.abs() + e_d) + e_d
    zero = torch.zeros_like(d)
    return torch.where(live, d, zero), torch.where(live, tol, zero), torch.where(live, e_d, zero)


def made_forward_outputs(f, V, pad_fill=1.0):
    """what a backward-only test hands to the kernel AND to the reference: the fp64 logits rounded once to bf16 (the padding
    columns filled with pad_fill: the kernel must write zeros there whatever it finds) and the fp64 lse rounded once to fp32"""
    R = f["z"].shape[0]
    x = torch.full((R, padded(V)), pad_fill, dtype=torch.bfloat16)
    x[:, :V] = f["z"].to(torch.bfloat16)
    return x, f["L"].float()


def grads(dl, h, w, V):
    """the three gradient GEMMs of fusion_ops._LMHeadCE.backward at the kernel's own bf16 dlogits dl (R, Vp), whose columns >= V
    are zero: (dH, tol) (R, D) -- an fp32 result of a Vp-long contraction cut over workgroups, then one bf16 rounding --,
    (dW, tol) (V, D) fp32 with the R-long contraction, (db, tol) (V,) the fp32 column sums"""
    Vp = dl.shape[1]
    q = dl[:, :V]
    r, e = G.bound(w.t(), q, f32=True, Kc=Vp)
    dh = (r, B8 * (r.abs() + e) + e)
    dw = G.bound(h.t(), q.t(), f32=True)
    s, ts = G.colsum_bound(dl)
    return dh, dw, (s[:V], ts[:V])


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def excess(out, ref, tol):
    """(worst |err| / tol over the elements with tol > 0, message or None).  `not (err <= tol)` fails, so NaN fails, and where
    tol is 0 anything but the reference's value fails; the message gives the count, the worst excess and the first offender."""
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


# ---- the whole-tensor norms of tests/test_gemm_gpu.py::test_lm_head_cross_entropy_vs_torch, restated -------------------------------
def old_norms_accept(kind, out, ref, seq=None):
    """kind "loss": the per-sequence loss (the rows summed in groups of `seq`; default: all rows one sequence) within 2e-3 of
    the largest; "logits": rel-L2 < 3e-3; "dlogits": rel-L2 < 2e-2 (what the old test asks of the three gradients that are
    linear in dlogits).  Not finite is not accepted."""
    out, ref = out.detach().double(), ref.detach().double()
    if not bool(torch.isfinite(out).all()):
        return False
    if kind == "loss":
        seq = seq or out.numel()
        o, r = out.view(-1, seq).sum(1), ref.view(-1, seq).sum(1)
        return bool((o - r).abs().max() <= 2e-3 * r.abs().max())
    rel = float((out - ref).norm() / (ref.norm() + 1e-20))
    return rel < {"logits": 3e-3, "dlogits": 2e-2}[kind]


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------
DEFECTS = ("zt_from_bf16", "stats_skip_last", "no_smoothing_term", "stale_max", "first_64_records", "no_inf_guard")


def _exp(x):
    """__expf / the epilogue's exp2 of x log2e, in fp32"""
    return torch.exp2(x * LOG2E)


def _merge(m, s, mo, so, guard=True, stale=False):
    """one merge of two online-softmax states as the epilogue shuffle and the combine write it"""
    mn = torch.maximum(m, mo)
    fa, fb = _exp(m - mn), _exp(mo - mn)
    if guard:
        zero = torch.zeros_like(fa)
        fa, fb = torch.where(m == -math.inf, zero, fa), torch.where(mo == -math.inf, zero, fb)
    s = s * fa + so * fb
    return (torch.where(mo > m, m, mn) if stale else mn), s


def emulate_forward(h, w, bias_pad, tgt, V, smoothing, defect=None):
    """(logits bf16 (R, Vp), loss f32, lse f32, z f32 (R, Vp): the logits before their one rounding) with the kernels' rounding
    points: fp32 accumulation in 16-wide K blocks (one MFMA each) and the fp32 bias add; per 128-entry half tile four lanes of
    32 entries (entry a 16 + q 4 + r of the half tile belongs to lane q) each taking the maximum, the serial sums of z and of
    exp2((z - m) log2e) over its valid entries, the xor-16 and xor-32 merges; the combine's lane g folding records g, g + 64,
    ... and the six xor shuffles 32 .. 1; m + log s; the loss line.  defect: one of DEFECTS or None."""
    assert defect is None or defect in DEFECTS
    R, D = h.shape
    Vp = bias_pad.numel()
    nrec = n_records(V)
    W = nrec * 128
    guard = defect != "no_inf_guard"
    hf = h.float()
    wf = torch.zeros(W, D, dtype=torch.float32)
    wf[:V] = w.float()
    acc = torch.zeros(R, W, dtype=torch.float32)
    for k in range(0, D, 16):
        acc = acc + hf[:, k:k + 16] @ wf[:, k:k + 16].t()
    bp = torch.zeros(W, dtype=torch.float32)
    bp[:Vp] = bias_pad
    z = acc + bp
    stored = z[:, :Vp].to(torch.bfloat16)
    n_valid = V - 1 if defect == "stats_skip_last" else V
    ninf = torch.tensor(-math.inf, dtype=torch.float32)
    zero = torch.tensor(0.0, dtype=torch.float32)
    # (R, record, a, lane q, r) -> (R, record, lane, 32 entries in the lane's order a, r)
    lanes = lambda t: t.reshape(-1, nrec, 8, 4, 4).permute(0, 1, 3, 2, 4).reshape(-1, nrec, 4, 32)
    zl = lanes(z)
    ok = lanes((torch.arange(W) < n_valid).expand(R, W))
    m = torch.where(ok, zl, ninf).amax(3)
    sz = torch.zeros(R, nrec, 4, dtype=torch.float32)
    se = torch.zeros(R, nrec, 4, dtype=torch.float32)
    for e in range(32):
        sz = sz + torch.where(ok[..., e], zl[..., e], zero)
    for e in range(32):
        se = se + torch.where(ok[..., e], torch.exp2((zl[..., e] - m) * LOG2E), zero)
    stale = defect == "stale_max"
    # xor 16: lanes (0, 1) and (2, 3); xor 32: (0, 2).  Lane 0 stores; its partner in the second step is lane 2's first merge
    m0, s0 = _merge(m[..., 0], se[..., 0], m[..., 1], se[..., 1], guard, stale)
    m2, s2 = _merge(m[..., 2], se[..., 2], m[..., 3], se[..., 3], guard, stale)
    pm, ps = _merge(m0, s0, m2, s2, guard, stale)
    pz = (sz[..., 0] + sz[..., 1]) + (sz[..., 2] + sz[..., 3])
    valid = tgt >= 0
    t = tgt.long().clamp(min=0)[:, None]
    zt = (stored.float() if defect == "zt_from_bf16" else z).gather(1, t)[:, 0]
    if defect == "stats_skip_last":
        zt = torch.where(tgt == V - 1, zero, zt)        # the target's lane never writes: the buffer's zero stays
    # combine: one wave per row
    use = min(nrec, 64) if defect == "first_64_records" else nrec
    cm = torch.full((R, 64), -math.inf, dtype=torch.float32)
    cs = torch.zeros(R, 64, dtype=torch.float32)
    cz = torch.zeros(R, 64, dtype=torch.float32)
    for g0 in range(0, use, 64):
        n = min(64, use - g0)
        mg, sg = pm[:, g0:g0 + n], ps[:, g0:g0 + n]
        cz[:, :n] = cz[:, :n] + pz[:, g0:g0 + n]
        mn = torch.maximum(cm[:, :n], mg)
        fa = _exp(cm[:, :n] - mn)
        if guard:
            fa = torch.where(cm[:, :n] == -math.inf, zero, fa)
        sn = cs[:, :n] * fa + sg * _exp(mg - mn)
        skip = (mg == -math.inf) if guard else torch.zeros_like(mg, dtype=torch.bool)
        cs[:, :n] = torch.where(skip, cs[:, :n], sn)
        cm[:, :n] = torch.where(skip, cm[:, :n], mn)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        o = lane ^ off
        cz = cz + cz[:, o]
        cm, cs = _merge(cm, cs, cm[:, o], cs[:, o], guard)
    lse = cm[:, 0] + torch.log(cs[:, 0])
    eps = torch.tensor(smoothing, dtype=torch.float32)
    ls = (1.0 - eps) * (lse - zt) + eps * (lse - cz[:, 0] / float(V))
    return stored, torch.where(valid, ls, zero), lse, z[:, :Vp]


def emulate_dlogits(x, l, g, tgt, V, smoothing, defect=None):
    """(dlogits bf16 (R, Vp), the fp32 values before their one rounding): the kernel's line in fp32"""
    assert defect is None or defect in DEFECTS
    R, Vp = x.shape
    eps = torch.tensor(smoothing, dtype=torch.float32)
    un = torch.zeros((), dtype=torch.float32) if defect == "no_smoothing_term" else eps / float(V)
    cols = torch.arange(Vp)[None, :]
    hot = cols == tgt.long()[:, None]
    d = _exp(x.float() - l.float()[:, None]) - un - torch.where(hot, 1.0 - eps, torch.zeros((), dtype=torch.float32))
    d = g.float()[:, None] * d
    live = (tgt >= 0)[:, None] & (cols < V)
    d = torch.where(live, d, torch.zeros_like(d))
    return d.to(torch.bfloat16), d
