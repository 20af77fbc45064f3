"""fp64 reference of the fused attention (csrc/attn.hip, csrc/attn_persist.hip) and the per-element bound its outputs are held
to: one wrong 32-row wave, one dropped 64-key tile or one wrong ragged row fails, where a whole-tensor norm would not notice.

The reference is built in fp64 from the bf16 inputs the kernel saw: S = scale Q K^T + mask (natural units, -inf where causal
hides a key), P = softmax(S), lse = log2-domain log-sum-exp, Z = keep / (1 - p) (all ones without dropout), P^ = P o Z,
O = P^ V; for a given dO: dP = dO V^T, D = rowsum(dO o O64), dS = P o (Z o dP - D), dQ = scale dS K, dK = scale dS^T Q,
dV = P^T dO.  Products with absolute values (|A| |B|) are fp64 as well.

Bound (u = 2^-24, C = 3; all products elementwise unless written as a matrix product):
    delta_ij = 64 u scale (|Q| |K|^T)_ij + 4 u (|s_ij| + |m_i| + ln Lk + 1)      exponent error of P_ij (natural units):
               the 64-term fp32 MFMA dot product, the fp32 fma with scale * log2(e) (itself rounded), the mask times log2(e)
               in fp32, the subtraction of the running max m_i / of the LSE (|lse| <= |m| + log2 Lk)
    sigma    = (ceil(Lk / 32) + 24) u                                               relative error of the fp32 row sum l:
               16 in-lane adds per 32-key block, one across the lane halves, one per block, up to 4 partial states merged
    rho_ij   = delta_ij + sum_j' P_ij' delta_ij' + sigma + 2^-22                    relative error of the kernel's P_ij:
               its own exponent, the error of the LSE / normaliser it is divided by, v_exp_f32 / v_log_f32
    O:   2^-8 |O64| + C [ (2^-8 + Lk u) (P^ |V|) + (P^ o rho) |V| ]                  bf16 P operand, fp32 accumulation (the
               rescales multiply the accumulator and the row sum by the same fp32 alpha, so their error cancels but for
               rounding), bf16 output
    LSE: C ( sum_j P_ij delta_ij log2 e + sigma log2 e + 2^-20 max(1, |lse64|) )
    dD_i = |sum_d dO (O_in - O64)| + 64 u sum_d |dO| |O_in|                         the kernel forms D from the STORED bf16 O
               (O_in).  The 2^-8 sum |dO| |O64| of a correctly rounded O would not cover it: the forward's own bound allows O
               to be off by C (2^-8 + Lk u) P^ |V|, many times 2^-8 |O64| on long rows, so this term is measured, not modelled
    E    = (2^-8 + rho) |dS| + P o (dD + 64 u Z o (|dO| |V|^T))                      bf16 dS, the recomputed P, the MFMA dP
    dQ:  2^-8 |dQ64| + C scale (E + Lk u |dS|) |K|
    dK:  2^-8 |dK64| + C scale (E + Lq u |dS|)^T |Q|
    dV:  2^-8 |dV64| + C ((2^-8 + rho + Lq u) o P^)^T |dO|
The 2^-8 terms take bf16 rounding (at most 2^-8 relative: 8 significant bits, round to nearest) of the operand or result they
stand beside; the C-multiplied terms are first-order error sums.  C = 3, not 2: where a row has ONE visible key (causal row 0,
a sample with a single unmasked key, Lq = 1 for dV) a product has one term and is rounded twice -- the bf16 operand P^ / dS by
up to 2^-8 and the bf16 result by up to 2^-8 -- so the error reaches 2 x 2^-8 |X|; with C = 2 the bound there is 3 x 2^-8 |X|
(a margin of 1.5, the CPU emulation reaches |err| / bound = 0.58), with C = 3 it is 4 x 2^-8 |X| (a margin of 2).  The second
-order products of small terms (rho times a rounding, the rounding of an already rounded sum) fit in the same factor.
tests/test_attn_bound_cpu.py shows the bound is not tighter than the arithmetic it models (a CPU emulation of the kernels'
rounding points passes with a margin of at least 2 on every element) and that it sees the defects a relative-L2 norm misses.

Not held: rows whose every visible key is masked (additive mask <= -1000).  Their softmax is defined by the masked scores
alone, which the kernel holds in fp32 at 14427 (-10000 log2 e) or 1.4e9 (-1e9 log2 e) -- one ulp there is 2^-10 or 128 in the
exponent -- so the kernel's answer is ill-defined to its own precision; dK / dV of a (batch, head) with such a row are not held
either.  A row with exactly one unmasked key IS held.
"""
import math

import torch

U = 2.0 ** -24
C = 3.0
B8 = 2.0 ** -8
LOG2E = 1.4426950408889634
MASKED = -1000.0   # additive mask values at or below this hide a key (med.py: -10000 or -1e9)


def _keep_mask(seed, B, H, Lq, Lk, p, dev, counter=None, keys=None):
    """The kernel's stateless dropout hash (attn_common.h drop_keep) restated with 64-bit integer tensors: keep[b, h, q, k].
    counter: the value of the seed_ptr device counter (effective seed (counter * 2654435761 + seed) mod 2^32, eff_seed);
    keys: the padded key index hashed for each key (two key segments: the second starts at 64 * ceil(Lk1 / 64))."""
    M = 0xFFFFFFFF
    if counter is not None:
        seed = (int(counter) * 2654435761 + int(seed)) & M
    bh = torch.arange(B * H, device=dev, dtype=torch.int64).view(B, H, 1, 1)
    q = torch.arange(Lq, device=dev, dtype=torch.int64).view(1, 1, Lq, 1)
    k = (torch.arange(Lk, device=dev, dtype=torch.int64) if keys is None else keys.to(dev, torch.int64)).view(1, 1, 1, Lk)
    x = (seed & M) ^ ((bh * 0x9E3779B1) & M) ^ ((q * 0x85EBCA77) & M) ^ ((k * 0xC2B2AE3D) & M)
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & M; x = x ^ (x >> 15); x = (x * 0x846ca68b) & M; x = x ^ (x >> 16)
    return x >= int(p * 4294967296.0)


def _bh(t):
    """(B, L, H, 64) -> fp64 (B * H, L, 64)"""
    B, L, H, D = t.shape
    return t.double().permute(0, 2, 1, 3).reshape(B * H, L, D)


def reference(q, k, v, scale, mask=None, causal=False, p=0.0, seed=0, counter=None, keys=None, dO=None, O_in=None,
              budget=1 << 23):
    """fp64 outputs and bounds.  q (B, Lq, H, 64), k / v (B, Lk, H, 64), dO like q, O_in the bf16 O the backward was given
    (default: O64 rounded to bf16); mask: additive key mask in natural units, (B, Lk) or None.  Chunked over (batch, head)
    so that about `budget` elements of each (Lq, Lk) matrix exist at once.  Returns a dict of (B, L, H, 64) / (B, H, Lq)
    fp64 tensors: O, tolO, lse, tolL and, with dO, dQ, tolQ, dK, tolK, dV, tolV (tolerances inf where not held)."""
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    G = B * H
    dev = q.device
    Q, K, V = _bh(q), _bh(k), _bh(v)
    G_ = _bh(dO) if dO is not None else None
    Oi = _bh(O_in) if O_in is not None else None
    Z = None
    if p > 0:
        Z = _keep_mask(seed, B, H, Lq, Lk, p, dev, counter, keys).reshape(G, Lq, Lk).double() / (1.0 - p)
    Mk = None
    if mask is not None:
        Mk = mask.double().reshape(B, 1, Lk).expand(B, H, Lk).reshape(G, 1, Lk).to(dev)
    sigma = (math.ceil(Lk / 32) + 24) * U
    out = {n: torch.empty(G, Lq, 64, dtype=torch.float64, device=dev) for n in ("O", "tolO")}
    out.update({n: torch.empty(G, Lq, dtype=torch.float64, device=dev) for n in ("lse", "tolL")})
    if dO is not None:
        out.update({n: torch.empty(G, Lq, 64, dtype=torch.float64, device=dev) for n in ("dQ", "tolQ")})
        out.update({n: torch.empty(G, Lk, 64, dtype=torch.float64, device=dev) for n in ("dK", "tolK", "dV", "tolV")})
    step = max(1, budget // (Lq * Lk))
    for g0 in range(0, G, step):
        g = slice(g0, min(G, g0 + step))
        Qg, Kg, Vg = Q[g], K[g], V[g]
        s = scale * (Qg @ Kg.transpose(1, 2))
        hidden = torch.zeros_like(s, dtype=torch.bool)
        if Mk is not None:
            s = s + Mk[g]
            hidden |= (Mk[g] <= MASKED).expand_as(s)
        if causal:
            fut = torch.ones(Lq, Lk, dtype=torch.bool, device=dev).triu(1)
            s = s.masked_fill(fut, -math.inf)
            hidden |= fut
        dead = hidden.all(-1)                                   # (g, Lq): no visible unmasked key
        m = s.amax(-1, keepdim=True)
        lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
        P = torch.exp(s - lse)
        delta = 64 * U * scale * (Qg.abs() @ Kg.abs().transpose(1, 2)) + 4 * U * (s.abs() + m.abs() + math.log(Lk) + 1.0)
        delta = torch.where(P > 0, delta, torch.zeros_like(delta))
        Pd = (P * delta).sum(-1, keepdim=True)
        rho = delta + Pd + sigma + 2.0 ** -22
        Ph = P * Z[g] if Z is not None else P
        O = Ph @ Vg
        tolO = B8 * O.abs() + C * ((B8 + Lk * U) * (Ph @ Vg.abs()) + (Ph * rho) @ Vg.abs())
        lse2 = lse[..., 0] * LOG2E
        tolL = C * (Pd[..., 0] * LOG2E + sigma * LOG2E + 2.0 ** -20 * lse2.abs().clamp(min=1.0))
        inf = torch.tensor(math.inf, dtype=torch.float64, device=dev)
        out["O"][g], out["tolO"][g] = O, torch.where(dead[..., None], inf, tolO)
        out["lse"][g], out["tolL"][g] = lse2, torch.where(dead, inf, tolL)
        del delta, tolO
        if dO is not None:
            Gg = G_[g]
            dP = Gg @ Vg.transpose(1, 2)
            D = (Gg * O).sum(-1, keepdim=True)
            Zg = Z[g] if Z is not None else 1.0
            dS = P * (Zg * dP - D)
            Og = Oi[g] if Oi is not None else O.to(torch.bfloat16).double()
            dD = (Gg * (Og - O)).sum(-1, keepdim=True).abs() + 64 * U * (Gg.abs() * Og.abs()).sum(-1, keepdim=True)
            E = (B8 + rho) * dS.abs() + P * (dD + 64 * U * Zg * (Gg.abs() @ Vg.abs().transpose(1, 2)))
            dQ, dK, dV = scale * (dS @ Kg), scale * (dS.transpose(1, 2) @ Qg), Ph.transpose(1, 2) @ Gg
            tolQ = B8 * dQ.abs() + C * scale * ((E + Lk * U * dS.abs()) @ Kg.abs())
            tolK = B8 * dK.abs() + C * scale * ((E + Lq * U * dS.abs()).transpose(1, 2) @ Qg.abs())
            tolV = B8 * dV.abs() + C * (((B8 + rho + Lq * U) * Ph).transpose(1, 2) @ Gg.abs())
            anydead = dead.any(-1)[:, None, None]
            out["dQ"][g], out["tolQ"][g] = dQ, torch.where(dead[..., None], inf, tolQ)
            out["dK"][g], out["tolK"][g] = dK, torch.where(anydead, inf, tolK)
            out["dV"][g], out["tolV"][g] = dV, torch.where(anydead, inf, tolV)
            del dP, dS, E
        del s, P, Ph, rho
    res = {}
    for n, t in out.items():
        if t.dim() == 3:
            res[n] = t.reshape(B, H, t.shape[1], 64).permute(0, 2, 1, 3)
        else:
            res[n] = t.reshape(B, H, Lq)
    return res


class _Checker:
    """collects every element outside its bound (the battery runs on; the test reports all of them) and the largest
    |err| / bound per (case, output)"""

    def __init__(self):
        self.failures, self.checked, self.ratios = [], 0, {}

    def __call__(self, name, out, ref, tol, route=None):
        out = out.detach().to(ref.device).double()
        skip = torch.isinf(tol)
        err = torch.where(skip, torch.zeros_like(ref), (out - ref).abs())
        bad = ~(err <= tol)
        self.checked += int((~skip).sum())
        held = ~skip & (tol > 0)
        r = float((err[held] / tol[held]).max()) if held.any() else 0.0
        if bad.any():
            r = max(r, math.inf if torch.isnan(out[bad]).any() else r)
        key = route or name
        self.ratios[key] = max(self.ratios.get(key, 0.0), r)
        if bad.any():
            idx = tuple(int(i) for i in bad.nonzero()[0])
            self.failures.append("%s: %d of %d elements out of bound, first at %s: out %r ref %r tol %r" % (
                name, int(bad.sum()), out.numel(), idx, float(out[idx]), float(ref[idx]), float(tol[idx])))
        return r

    def check_all(self, name, got, ref, route=None):
        """got: {"O", "lse", "dQ", "dK", "dV"} (any subset) against reference()'s result"""
        tols = {"O": "tolO", "lse": "tolL", "dQ": "tolQ", "dK": "tolK", "dV": "tolV"}
        for n, t in got.items():
            self("%s.%s" % (name, n), t, ref[n], ref[tols[n]], route=(route + "." + n) if route else None)
