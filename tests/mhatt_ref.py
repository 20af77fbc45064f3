"""Reference, bounds, fp32 restatement and inputs of the kernels of csrc/mhatt.hip (include/bqhip_mhatt.h): the attention core of
MHAtt -- scores, fill, softmax, dropout multiplier, the product with V -- forward and backward, for tests/test_mhatt_cpu.py and
tests/test_mhatt_gpu.py.  Nothing here needs a GPU or the extension.

LAYOUT.  q (B, Nq, heads d), k, v (B, Nk, heads d), dout and out as q: head h of a row is its columns [h d, (h + 1) d).
hide (B, Nk) bool, True = hidden key, or None.  keep (B, heads, Nq, Nk) fp32, 0 or 1 / (1 - p_drop), or None.
p and ds are (B, heads, Nq, Nk).

REFERENCE.  fp64 from the fp32 operands the kernels see; sqrt(d) is the fp32 value sqrtf(d).
    forward    a = sum_c q k, s = a / sqrt d, l = hide ? -1e9 : s (fp32(-1e9) is exactly -1e9), p = softmax_j(l),
               out = sum_j (p keep) v
    backward   p GIVEN (fp32, as the kernel reads it): g = sum_c dout v, dp = keep g, t = sum_j p dp,
               ds = hide ? 0 : p (dp - t), dq = (sum_j ds k) / sqrt d, dk = (sum_i ds q) / sqrt d, dv = sum_i (p keep) dout

BOUNDS, per element, first order, for ANY order of a sum.  u = 2^-24, Du = (d + 8) u, Ku = (Nk + 8) u, Qu = (Nq + 8) u: a sum of
K fp32 terms errs by at most (K - 1) u sum|terms|, and the 8 covers the elementwise roundings around each sum.
    s      e_s = Du sum_c |q k| / sqrt d + 2 u |s|                      (0 at hidden keys: the fill is exact)
    p      the error of a logit moves p_j by p_j (e_s[j] + sum_k p_k e_s[k]); the rounding of l - max is an absolute error
           u |l - max| of the exponent, expf is 1 ulp, the Nk positive terms, the division:
           rel_p[j] = e_s[j] + sum_k p_k e_s[k] + (|l_j - max| + Nk + 16) u,   tol_p = p rel_p, plus 2^-126 on visible keys (a
           flushed denormal).  A hidden key next to a visible one has p = 0 exactly, in fp32 and in fp64 alike, tolerance 0.
    out    tol_out = sum_j |p keep v| (rel_p[j] + u + Ku)                (u: the product p keep)
    g      e_g = Du sum_c |dout v|
    dp     e_dp = keep e_g + u |dp|
    t      e_t = Ku sum_j |p dp| + sum_j p e_dp
    ds     e_ds = p (e_dp + e_t + u (|dp| + |t|)) + u |ds|               (0 at hidden keys)
    dq     (Ku sum_j |ds k| + sum_j e_ds |k|) / sqrt d + 3 u |dq|
    dk     (Qu sum_i |ds q| + sum_i e_ds |q|) / sqrt d + 3 u |dk|
    dv     (Qu + u) sum_i |p keep dout|
Where a tolerance is 0 the result must be exact (ln_ref.excess holds `err <= tol`): a hidden key next to a visible one (p, dk,
dv), a fully hidden sample's dq and dk, a query whose keep row is all zero (out, and its share of everything downstream).

RESTATEMENT.  The same arithmetic in fp32 tensors on the host with the kernels' rounding points and order of additions: the dot
products are chains from 0 over ascending c, the softmax denominator and t are formed as a wave forms them (lane n adds its keys
n, n + 64, ... in ascending order, the 64 lane sums are folded by halves), the products with V, K (over j) and with q, dout
(over i) are chains from 0 in ascending order.  Only expf may differ from the device in the last bit.  `defect` plants one named
error for tests/test_mhatt_cpu.py.
"""
import functools
import math
import zlib

import torch

from ln_ref import excess  # noqa: F401  (the per-element comparison, shared)

U = 2.0 ** -24
FILL = -1e9
TINY = 2.0 ** -126
P_DROP = 0.1

SHAPES = [(1, 1, 1, 1, 32), (3, 2, 5, 9, 32), (3, 8, 37, 9, 32), (3, 3, 67, 130, 32), (3, 2, 70, 257, 64), (3, 1, 3, 1024, 32),
          (2, 1, 1024, 5, 32)]
MASKS = ("none", "mixed")
KEEPS = (False, True)
CASES = [(s, m, kp) for s in SHAPES for m in MASKS for kp in KEEPS if m == "none" or s[0] == 3]
DEFECTS = ("no_scale", "fill_inf", "no_zero", "t_from_g", "p_bf16")


def case_id(case):
    (B, heads, Nq, Nk, d), kind, kp = case
    return "%dx%dx%dx%dx%d-%s-%s" % (B, heads, Nq, Nk, d, kind, "keep" if kp else "nokeep")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def sqrt_d(d):
    """sqrtf(d) as a Python float"""
    return float(torch.tensor(float(d), dtype=torch.float32).sqrt())


def split(x, heads):
    """(B, N, heads d) -> (B, heads, N, d), a view"""
    B, N, H = x.shape
    return x.view(B, N, heads, H // heads).transpose(1, 2)


def merge(x):
    """(B, heads, N, d) -> (B, N, heads d)"""
    B, heads, N, d = x.shape
    return x.transpose(1, 2).reshape(B, N, heads * d)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_hide(B, Nk, kind):
    """bool (B, Nk), True = hidden, or None.  "mixed" (B = 3): sample 0 has its tail hidden (the last third), sample 1 is hidden
    completely, sample 2 shows the single key Nk // 2"""
    if kind == "none":
        return None
    assert kind == "mixed" and B == 3
    hide = torch.zeros(B, Nk, dtype=torch.bool)
    hide[0, Nk - Nk // 3:] = True
    hide[1] = True
    hide[2] = True
    hide[2, Nk // 2] = False
    return hide


@functools.lru_cache(maxsize=None)
def keep_scale():
    """the fp32 value 1 / (1 - 0.1) as torch's dropout forms it"""
    with torch.random.fork_rng():
        torch.manual_seed(0)
        return float(torch.nn.functional.dropout(torch.ones(256), P_DROP, training=True).max())


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, with_keep):
    """dict of q, k, v, dout (fp32), hide, keep, heads, seeded by the shape: q, k ~ 1.5 N(0, 1), v, dout ~ N(0, 1) -- the visible
    logits stay within 40 of their row maximum, so expf does not underflow; keep drawn at 0.1 with keep[0, 0, 0, :] = 0.
    Shared between tests: do not write to the tensors."""
    B, heads, Nq, Nk, d = shape
    H = heads * d
    g = torch.Generator().manual_seed(_seed("mhatt", shape))
    q = torch.randn(B, Nq, H, generator=g) * 1.5
    k = torch.randn(B, Nk, H, generator=g) * 1.5
    v = torch.randn(B, Nk, H, generator=g)
    dout = torch.randn(B, Nq, H, generator=g)
    keep = None
    if with_keep:
        keep = (torch.rand(B, heads, Nq, Nk, generator=g) >= P_DROP).float() * keep_scale()
        keep[0, 0, 0, :] = 0.0
    return dict(q=q, k=k, v=v, dout=dout, hide=make_hide(B, Nk, kind), keep=keep, heads=heads)


# ---- reference and bounds -------------------------------------------------------------------------------------------------------
def _hid(hide):
    return hide[:, None, None, :]


def forward(q, k, v, hide, keep, heads):
    """fp64 p (B, heads, Nq, Nk), out (B, Nq, H) with tol_p, tol_out"""
    d, Nk = q.shape[2] // heads, k.shape[1]
    Du, Ku, sq = (d + 8) * U, (Nk + 8) * U, sqrt_d(d)
    qd, kd, vd = split(q.double(), heads), split(k.double(), heads), split(v.double(), heads)
    s = torch.einsum("bhic,bhjc->bhij", qd, kd) / sq
    e_s = Du * torch.einsum("bhic,bhjc->bhij", qd.abs(), kd.abs()) / sq + 2.0 * U * s.abs()
    floor = torch.full_like(s, TINY)
    if hide is not None:
        s = s.masked_fill(_hid(hide), FILL)
        e_s = e_s.masked_fill(_hid(hide), 0.0)
        floor = floor.masked_fill(_hid(hide), 0.0)
    p = torch.softmax(s, dim=-1)
    rel_p = e_s + (p * e_s).sum(-1, keepdim=True) + ((s - s.amax(-1, keepdim=True)).abs() + Nk + 16) * U
    w = p if keep is None else p * keep.double()
    out = torch.einsum("bhij,bhjc->bhic", w, vd)
    tol_out = torch.einsum("bhij,bhjc->bhic", w.abs() * (rel_p + U + Ku), vd.abs())
    return dict(p=p, out=merge(out), tol_p=p * rel_p + floor, tol_out=merge(tol_out))


def backward(dout, q, k, v, p, hide, keep, heads):
    """fp64 dq, dk, dv (as q, k, v) with tol_dq, tol_dk, tol_dv, and ds (B, heads, Nq, Nk).  p: the fp32 tensor the kernel reads."""
    d, Nq, Nk = q.shape[2] // heads, q.shape[1], k.shape[1]
    Du, Ku, Qu, sq = (d + 8) * U, (Nk + 8) * U, (Nq + 8) * U, sqrt_d(d)
    qd, kd, vd, dd = [split(t.double(), heads) for t in (q, k, v, dout)]
    pd = p.double()
    kp = torch.ones_like(pd) if keep is None else keep.double()
    g = torch.einsum("bhic,bhjc->bhij", dd, vd)
    e_g = Du * torch.einsum("bhic,bhjc->bhij", dd.abs(), vd.abs())
    dp = kp * g
    e_dp = kp * e_g + U * dp.abs()
    t = (pd * dp).sum(-1, keepdim=True)
    e_t = Ku * (pd * dp).abs().sum(-1, keepdim=True) + (pd * e_dp).sum(-1, keepdim=True)
    ds = pd * (dp - t)
    e_ds = pd * (e_dp + e_t + U * (dp.abs() + t.abs())) + U * ds.abs()
    if hide is not None:
        ds = ds.masked_fill(_hid(hide), 0.0)
        e_ds = e_ds.masked_fill(_hid(hide), 0.0)
    dq = torch.einsum("bhij,bhjc->bhic", ds, kd) / sq
    tol_dq = (Ku * torch.einsum("bhij,bhjc->bhic", ds.abs(), kd.abs()) + torch.einsum("bhij,bhjc->bhic", e_ds, kd.abs())) / sq \
        + 3.0 * U * dq.abs()
    dk = torch.einsum("bhij,bhic->bhjc", ds, qd) / sq
    tol_dk = (Qu * torch.einsum("bhij,bhic->bhjc", ds.abs(), qd.abs()) + torch.einsum("bhij,bhic->bhjc", e_ds, qd.abs())) / sq \
        + 3.0 * U * dk.abs()
    w = pd * kp
    dv = torch.einsum("bhij,bhic->bhjc", w, dd)
    tol_dv = (Qu + U) * torch.einsum("bhij,bhic->bhjc", w.abs(), dd.abs())
    return dict(dq=merge(dq), dk=merge(dk), dv=merge(dv), ds=ds, tol_dq=merge(tol_dq), tol_dk=merge(tol_dk), tol_dv=merge(tol_dv))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, forward reference, p32 = the reference's p rounded once to fp32 -- what a backward test hands to the kernel AND to
    the reference --, backward reference) of a case of CASES; computed once, read-only"""
    shape, kind, kp = case
    d = inputs(shape, kind, kp)
    fwd = forward(d["q"], d["k"], d["v"], d["hide"], d["keep"], d["heads"])
    p32 = fwd["p"].float()
    bwd = backward(d["dout"], d["q"], d["k"], d["v"], p32, d["hide"], d["keep"], d["heads"])
    return d, fwd, p32, bwd


# ---- the torch composition of bridgeqa_amd/mcan_module.py as it stood before the fused route: what "unchanged" means --------------
def composition_mhatt(m, v, k, q, mask):
    B = q.size(0)
    v, k, q = m._split(m.linear_v(v), B), m._split(m.linear_k(k), B), m._split(m.linear_q(q), B)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(q.size(-1))
    if mask is not None:
        scores = scores.masked_fill(mask, -1e9)
    ctx = torch.matmul(m.dropout(torch.softmax(scores, dim=-1)), v)
    return m.linear_merge(ctx.transpose(1, 2).contiguous().view(B, -1, m.hidden_size))


# ---- fp32 restatement of the kernels' arithmetic --------------------------------------------------------------------------------
def _fold64(s):
    """(..., 64) lane values -> (..., 1): the xor butterfly 32, 16, .. 1 adds halves"""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s


def _wave_sum(v):
    """sums over the last axis as one wave forms them: lane n adds its values n, n + 64, ... in ascending order, from 0"""
    v = torch.nn.functional.pad(v, (0, -v.shape[-1] % 64))
    t = v.reshape(v.shape[:-1] + (v.shape[-1] // 64, 64))
    s = torch.zeros(v.shape[:-1] + (64,), dtype=torch.float32)
    for i in range(t.shape[-2]):
        s = s + t[..., i, :]
    return _fold64(s)


def _dots(x, y):
    """(B, h, Nx, d), (B, h, Ny, d) -> (B, h, Nx, Ny): one product per term, a chain from 0 over ascending c"""
    a = torch.zeros(x.shape[:3] + (y.shape[2],), dtype=torch.float32)
    for c in range(x.shape[3]):
        a = a + x[:, :, :, None, c] * y[:, :, None, :, c]
    return a


def _chain(w, y):
    """(B, h, Nx, Ny), (B, h, Ny, d) -> (B, h, Nx, d): sum over the Ny axis, a chain from 0 in ascending order"""
    acc = torch.zeros(w.shape[:3] + (y.shape[3],), dtype=torch.float32)
    for j in range(w.shape[3]):
        acc = acc + w[:, :, :, j, None] * y[:, :, None, j, :]
    return acc


def _scale(d):
    return torch.tensor(float(d), dtype=torch.float32).sqrt()


def emulate_forward(q, k, v, hide, keep, heads, defect=None):
    """out (B, Nq, H), p (B, heads, Nq, Nk) in fp32.  defect: "no_scale", "fill_inf", "p_bf16" """
    d = q.shape[2] // heads
    qh, kh, vh = split(q, heads), split(k, heads), split(v, heads)
    a = _dots(qh, kh)
    s = a if defect == "no_scale" else a / _scale(d)
    if hide is not None:
        s = s.masked_fill(_hid(hide), float("-inf") if defect == "fill_inf" else FILL)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = e / _wave_sum(e)
    if defect == "p_bf16":
        p = p.to(torch.bfloat16).float()
    w = p if keep is None else p * keep
    return merge(_chain(w, vh)), p


def emulate_backward(dout, q, k, v, p, hide, keep, heads, defect=None):
    """dq, dk, dv in fp32 from p as given.  defect: "no_zero" (ds not zeroed under the mask), "t_from_g" (t from g, not keep g)"""
    d = q.shape[2] // heads
    qh, kh, vh, dh = split(q, heads), split(k, heads), split(v, heads), split(dout, heads)
    g = _dots(dh, vh)
    dp = g if keep is None else keep * g
    t = _wave_sum(p * (g if defect == "t_from_g" else dp))
    ds = p * (dp - t)
    if hide is not None and defect != "no_zero":
        ds = ds.masked_fill(_hid(hide), 0.0)
    sc = _scale(d)
    dq = _chain(ds, kh) / sc
    dk = _chain(ds.transpose(2, 3), qh) / sc
    w = p if keep is None else p * keep
    dv = _chain(w.transpose(2, 3), dh)
    return merge(dq), merge(dk), merge(dv)
