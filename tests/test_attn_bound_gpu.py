"""Every kernel route of the fused attention (csrc/attn.hip bq_attn_fwd / bq_attn_bwd / pair / two-segment / probs,
csrc/attn_persist.hip) held ELEMENTWISE to the fp64 bound of tests/attn_ref.py, on every output it produces (O, LSE, dQ, dK,
dV, P): one wrong 32-row wave, one dropped key tile or one wrong ragged row fails where the relative-L2 norms of
tests/test_attn_gpu.py do not.  Each case names the kernels it must reach and proves it: the case runs once under
torch.profiler and the set of attention kernels launched must equal the expected set (the persist thresholds use the CU count
of torch.cuda.get_device_properties).  Operands come as the product passes them (q / k / v slices of (B, L, 3, H, 64), k / v
of (B, L, 2, H, 64)); gradients go into strided views of NaN-filled buffers whose other slots must stay NaN.  Dropout is
seeded through a device counter (seed_tensor) and through the scalar seed.  The resident-grid switch is run through all
eight masks and bit 3 (scalar softmax) at the ViT shape, and the matrix-path rows of the backward are asserted bit-equal to
mask 0's.

    python tests/test_attn_bound_gpu.py OUT.pt   runs the battery in this process (the test's child)
"""
import math
import os
import re
import subprocess
import sys
import time
import zlib

import pytest
import torch

from attn_ref import _Checker, _keep_mask, reference
from load_util import _repeat_under_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SCALE = 0.125
SEED = 4242
COUNTER = 77   # value of the seed_tensor device counter where a case draws its dropout through it

# ---- routes -----------------------------------------------------------------------------------------------------------------
_KNAME = re.compile(r"(attn_[a-z0-9_]*?kernel)(?:<([^>]*)>|I((?:L[a-z]\d+E)+)E)?")


def kernel_ids(names):
    """canonical ids ('attn_fwd_kernel<3,1>', 'attn_bwd_small_kernel') of the attention kernels among profiler kernel names,
    demangled ('bq::attn_fwd_kernel<3, true>') or not ('_ZN2bq15attn_fwd_kernelILi3ELi1EEEv...')"""
    out = set()
    for n in names:
        for m in _KNAME.finditer(n):
            base, dem, man = m.groups()
            if dem is not None:
                args = [{"true": "1", "false": "0"}.get(a.strip(), a.strip()) for a in dem.split(",")]
            elif man is not None:
                args = re.findall(r"L[a-z](\d+)E", man)
            else:
                args = []
            out.add(base + ("<%s>" % ",".join(args) if args else ""))
    return out


def _persist_ok(BH, nb, slots, hi):
    return BH % 8 == 0 and slots % 8 == 0 and BH * nb >= slots and BH * nb <= hi * slots


def routes(B, H, Lq, Lk, plain, persist, cus, backward=True):
    """the kernels bq_attn_fwd / bq_attn_bwd launch for this problem: the route table of csrc/attn.hip, restated"""
    BH = B * H
    if Lq <= 32 and Lk > 128:
        fwd = {"attn_fwd_narrow_kernel"}
    elif plain and persist & 1 and _persist_ok(BH, Lq // 128 + (1 if Lq % 128 > 1 else 0), 3 * cus, 4):
        fwd = {"attn_fwd_persist_kernel<3,%d>" % (0 if persist & 8 else 1)}
    else:
        fwd = {"attn_fwd_kernel<3,%d>" % (1 if plain else 0)}
    if not backward:
        return fwd
    if not plain and Lq <= 128 and Lk <= 128:
        return fwd | {"attn_bwd_small_kernel"}
    if plain and persist & 2 and _persist_ok(BH, Lq // 128 + (1 if Lq % 128 > 1 else 0), 3 * cus, 4):
        dq = "attn_bwd_dq_persist_kernel<3>"
    elif Lq <= 32 and Lk > 128:
        dq = "attn_bwd_dq_narrow_kernel"
    else:
        dq = "attn_bwd_dq_kernel<4,1>" if plain else "attn_bwd_dq_kernel<2,0>"
    if plain and persist & 4 and Lq > 64 and _persist_ok(BH, Lk // 128 + (1 if Lk % 128 > 1 else 0), 2 * cus, 6):
        dkv = "attn_bwd_dkv_persist_kernel<2>"
    else:
        dkv = "attn_bwd_dkv_kernel<2,%d>" % (1 if plain else 0)
    return fwd | {dq, dkv}


def profiled(fn):
    """fn() once under torch.profiler; returns (fn's result, attention kernel ids, number of device kernels seen)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return res, kernel_ids(names), len(names)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _mask(B, Lk, kind, dev, seed):
    """additive key mask, natural units (B, Lk): m4 / m9 = the -10000 / -1e9 conventions of med.py with sample 0's second half
    masked and (B > 1) a sample with a single unmasked key; soft = a graded bias in [-3, 0]"""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed)
    if kind == "soft":
        return (-3.0 * torch.rand(B, Lk, generator=g)).to(dev)
    big = -10000.0 if kind == "m4" else -1e9
    m = torch.zeros(B, Lk)
    m[0, max(1, Lk // 2):] = big
    if B > 1:
        m[-1, :] = big
        m[-1, Lk // 3] = 0.0
    return m.to(dev)


def _operands(B, H, Lq, Lk, dev, seed, spike):
    """q / k / v as the product passes them: self-attention (Lq == Lk) slices of one (B, L, 3, H, 64) tensor;
    otherwise q slot 0 of a (B, Lq, 3, H, 64) tensor and k / v slices of a (B, Lk, 2, H, 64) one"""
    g = torch.Generator().manual_seed(seed)
    self_attn = Lq == Lk
    if self_attn:
        X = torch.randn(B, Lq, 3, H, 64, generator=g) * 1.5
        X[:, :, 2] /= 1.5
        Xq, Xkv, kslot = X, X, 1
    else:
        Xq = torch.randn(B, Lq, 3, H, 64, generator=g) * 1.5
        Xkv = torch.randn(B, Lk, 2, H, 64, generator=g) * 1.5
        Xkv[:, :, 1] /= 1.5
        kslot = 0
    if spike:   # a late max jump: the last key aligned with the queries of the last row block
        r0 = max(0, Lq - 32)
        Xkv[:, Lk - 1, kslot] = Xq[:, r0:, 0].mean(1) * 6.0
    dO = torch.randn(B, Lq, H, 64, generator=g).to(dev).to(torch.bfloat16)
    Xq = Xq.to(dev).to(torch.bfloat16)
    Xkv = Xq if self_attn else Xkv.to(dev).to(torch.bfloat16)
    return Xq[:, :, 0], Xkv[:, :, kslot], Xkv[:, :, kslot + 1], dO, self_attn


def _nan_grads(q, k, self_attn):
    """dq / dk / dv views strided like q / k inside NaN buffers with a batch of slack on either side"""
    Xq = q._base
    Xk = k._base
    gq = torch.full((Xq.shape[0] + 2,) + tuple(Xq.shape[1:]), math.nan, device=q.device, dtype=torch.bfloat16)
    gk = gq if self_attn else torch.full((Xk.shape[0] + 2,) + tuple(Xk.shape[1:]), math.nan, device=q.device,
                                         dtype=torch.bfloat16)
    inner_q, inner_k = gq[1:-1], gk[1:-1]
    if self_attn:
        return (gq, gk), inner_q[:, :, 0], inner_q[:, :, 1], inner_q[:, :, 2], [(gq, (slice(1, -1), slice(None), slice(0, 3)))]
    return (gq, gk), inner_q[:, :, 0], inner_k[:, :, 0], inner_k[:, :, 1], [(gq, (slice(1, -1), slice(None), slice(0, 1))),
                                                                               (gk, (slice(1, -1), slice(None), slice(0, 2)))]


def _neighbours_nan(written):
    """every element of the buffers outside the written slots is still NaN"""
    for buf, (bs, ls, ss) in written:
        keep = torch.ones(buf.shape[:3], dtype=torch.bool, device=buf.device)
        keep[bs, ls, ss] = False
        rest = buf[keep]
        if not torch.isnan(rest.float()).all():
            return False
        if torch.isnan(buf[bs, ls, ss].float()).any():
            return False
    return True


# ---- the battery ------------------------------------------------------------------------------------------------------------
class Battery:
    def __init__(self, dev):
        from bridgeqa_amd import _ext
        self.ext, self.dev = _ext, dev
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.chk = _Checker()
        self.seen = set()
        self.log = []

    def fail(self, msg):
        self.chk.failures.append(msg)

    def expect(self, name, want, got, ndev):
        self.seen |= got
        if ndev == 0:
            self.fail("%s: the profiler reported no device kernels at all -- route coverage cannot be proven" % name)
        elif got != want:
            self.fail("%s: launched %s, expected %s" % (name, sorted(got), sorted(want)))

    def case(self, name, B, H, Lq, Lk, mask=None, causal=False, p=0.0, counter=True, spike=False, persist=0,
             backward=True, route=None):
        ext, dev = self.ext, self.dev
        q, k, v, dO, self_attn = _operands(B, H, Lq, Lk, dev, zlib.crc32(name.encode()) & 0xFFFF, spike)
        mk = _mask(B, Lk, mask, dev, Lk)
        ml2 = ext.key_mask_log2(mk.view(B, 1, 1, Lk), B, Lk) if mk is not None else None
        st = torch.tensor([COUNTER], dtype=torch.int32, device=dev) if (p > 0 and counter) else None
        plain = mk is None and not causal and p == 0
        prev = ext.attn_set_persistent(persist)
        try:
            bufs, dq, dk, dv, written = _nan_grads(q, k, self_attn)

            def run():
                out, lse = ext.attn_fwd(q, k, v, SCALE, ml2, p, SEED, st, causal)
                if backward:
                    ext.attn_bwd(q, k, v, out, lse, dO, SCALE, dq, dk, dv, ml2, p, SEED, st, causal)
                return out, lse
            (out, lse), got, ndev = profiled(run)
        finally:
            ext.attn_set_persistent(prev)
        self.expect(name, routes(B, H, Lq, Lk, plain, persist, self.cus, backward), got, ndev)
        ref = reference(q, k, v, SCALE, mk, causal, p, SEED, COUNTER if st is not None else None,
                        dO=dO if backward else None, O_in=out)
        res = {"O": out, "lse": lse}
        if backward:
            res.update(dQ=dq, dK=dk, dV=dv)
            if not _neighbours_nan(written):
                self.fail("%s: a gradient write left its slice (a NaN neighbour slot was overwritten) or missed an element" % name)
        self.chk.check_all(name, res, ref, route=route or name)
        self.log.append((name, sorted(got)))
        return res

    # -- the route table ----------------------------------------------------------------------------------------------------
    def extents(self):
        for L in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1025):
            self.case("plain.L%d" % L, 2, 3, L, L, route="plain")
            self.case("m4.L%d" % L, 2, 3, L, L, mask="m4", route="masked")
        self.case("plain.L4097", 1, 2, 4097, 4097, route="plain")
        for Lq in (1, 2, 20, 31, 32):
            for Lk in (129, 161, 276, 1045):
                self.case("narrow.plain.%dx%d" % (Lq, Lk), 2, 3, Lq, Lk, route="narrow")
            self.case("narrow.m9.%dx1045" % Lq, 2, 3, Lq, 1045, mask="m9", p=0.1, route="narrow")
        for Lq, Lk in ((33, 129), (32, 128), (33, 128), (32, 65), (65, 33), (200, 97), (129, 1025), (1025, 129)):
            self.case("cross.plain.%dx%d" % (Lq, Lk), 2, 3, Lq, Lk, route="cross")
            self.case("cross.m4.%dx%d" % (Lq, Lk), 2, 3, Lq, Lk, mask="m4", route="cross")

    def edges(self):
        # a late max jump on every forward route
        self.case("spike.narrow", 2, 3, 20, 1045, spike=True, route="spike")
        self.case("spike.plain", 2, 3, 300, 300, spike=True, route="spike")
        self.case("spike.general", 2, 3, 300, 300, mask="soft", spike=True, route="spike")
        self.case("spike.persist", 16, 12, 1025, 1025, spike=True, persist=1, backward=False, route="spike")
        # causal (decoder self-attention; training uses attention_probs_dropout_prob 0.1)
        for L in (5, 129, 257, 300):
            for p in (0.0, 0.1):
                self.case("causal.L%d.p%g" % (L, p), 2, 3, L, L, mask="m4" if L == 300 else None, causal=True, p=p,
                          route="causal")
        # masks: both conventions, a graded one, a single unmasked key (sample B - 1 of m4 / m9)
        for kind in ("m4", "m9", "soft"):
            self.case("mask.%s.L200" % kind, 3, 2, 200, 200, mask=kind, route="masked")
            self.case("mask.%s.20x276" % kind, 3, 2, 20, 276, mask=kind, route="narrow")
            self.case("mask.%s.L100" % kind, 3, 2, 100, 100, mask=kind, route="small")
        # dropout through the device counter and through the scalar seed
        for p in (0.1, 0.5):
            for ctr in (True, False):
                tag = "ctr" if ctr else "seed"
                self.case("drop.%s.p%g.L150" % (tag, p), 2, 3, 150, 150, p=p, counter=ctr, route="dropout")
                self.case("drop.%s.p%g.20x1045" % (tag, p), 2, 3, 20, 1045, mask="m4", p=p, counter=ctr, route="dropout")
                self.case("drop.%s.p%g.L20" % (tag, p), 2, 3, 20, 20, p=p, counter=ctr, route="dropout")

    def persist_masks(self):
        """the resident-grid switch at the ViT shape: every mask held to the bound; the backward of each mask, given mask 0's
        O / LSE, bit-equal to mask 0's on the matrix-path rows (all but the 1025th row / key)"""
        ext, dev = self.ext, self.dev
        B, H, L = 16, 12, 1025
        base = None
        for mask in (0, 1, 2, 3, 4, 5, 6, 7, 9, 15):
            name = "persist.%d" % mask
            self.case(name, B, H, L, L, persist=mask, route="persist")
            if base is None:
                q0, k0, v0, dO0, _ = _operands(B, H, L, L, dev, 12345, False)
                prev = ext.attn_set_persistent(0)
                try:
                    o0, l0 = ext.attn_fwd(q0, k0, v0, SCALE)
                finally:
                    ext.attn_set_persistent(prev)
                base = (q0, k0, v0, dO0, o0, l0, None)
            q0, k0, v0, dO0, o0, l0, g0 = base
            prev = ext.attn_set_persistent(mask)
            try:
                g = torch.empty(B, L, 3, H, 64, device=dev, dtype=torch.bfloat16)
                ext.attn_bwd(q0, k0, v0, o0, l0, dO0, SCALE, g[:, :, 0], g[:, :, 1], g[:, :, 2])
            finally:
                ext.attn_set_persistent(prev)
            if g0 is None:
                base = base[:6] + (g,)
            elif not torch.equal(g[:, :L - 1], g0[:, :L - 1]):
                d = (g[:, :L - 1] != g0[:, :L - 1]).nonzero()[0].tolist()
                self.fail("%s: backward rows 0..%d not bit-equal to mask 0 (first difference at %s)" % (name, L - 2, d))

    def pair(self):
        """bq_attn_fwd_pair / bq_attn_bwd_pair held to fp64 (twin cross-attentions: 1045 and 276 keys, masks, dropout with
        per-side seeds through the device counter)"""
        ext, dev = self.ext, self.dev
        B, H, Lq = 3, 4, 20
        st = torch.tensor([COUNTER], dtype=torch.int32, device=dev)
        for p in (0.0, 0.1):
            sides, refs_in = [], []
            for s_, Lk in enumerate((1045, 276)):
                q, k, v, dO, _ = _operands(B, H, Lq, Lk, dev, 900 + s_, False)
                mk = _mask(B, Lk, "m4", dev, Lk)
                sides.append(dict(q=q, k=k, v=v, out=torch.empty(B, Lq, H, 64, device=dev, dtype=torch.bfloat16),
                                  mask_log2=ext.key_mask_log2(mk.view(B, 1, 1, Lk), B, Lk), seed=SEED + s_))
                refs_in.append((q, k, v, dO, mk))
            grads = [_nan_grads(r[0], r[1], False) for r in refs_in]

            def run():
                lses = ext.attn_fwd_pair(sides, SCALE, p, st)
                bs = [dict(sides[s_], lse=lses[s_], grad_out=refs_in[s_][3], dq=grads[s_][1], dk=grads[s_][2], dv=grads[s_][3])
                      for s_ in range(2)]
                ext.attn_bwd_pair(bs, SCALE, p, st)
                return lses
            lses, got, ndev = profiled(run)
            name = "pair.p%g" % p
            self.expect(name, {"attn_fwd_narrow_pair_kernel", "attn_bwd_dq_narrow_pair_kernel", "attn_bwd_dkv_pair_kernel"},
                        got, ndev)
            for s_ in range(2):
                q, k, v, dO, mk = refs_in[s_]
                ref = reference(q, k, v, SCALE, mk, False, p, SEED + s_, COUNTER, dO=dO, O_in=sides[s_]["out"])
                if not _neighbours_nan(grads[s_][4]):
                    self.fail("%s side %d: a gradient write left its slice" % (name, s_))
                self.chk.check_all("%s.side%d" % (name, s_), dict(O=sides[s_]["out"], lse=lses[s_], dQ=grads[s_][1],
                                                                  dK=grads[s_][2], dV=grads[s_][3]), ref, route="pair")

    def two_segments(self):
        """bq_attn_fwd2 / bq_attn_bwd2: keys cat(segment 1, segment 2) without the concatenation (public ABI)"""
        ext, dev = self.ext, self.dev
        for n, (B, H, Lq, L1, L2, mask, p) in enumerate([(2, 3, 20, 1025, 20, "m4", 0.1), (2, 2, 7, 276, 33, None, 0.0)]):
            q, k1, v1, dO, _ = _operands(B, H, Lq, L1, dev, 950 + n, False)
            _, k2, v2, _, _ = _operands(B, H, Lq, L2, dev, 960 + n, False)
            mk = _mask(B, L1 + L2, mask, dev, 7) if mask else None
            ml = ext.key_mask_log2_two(mk.view(B, 1, 1, L1 + L2), B, L1, L2) if mk is not None else None
            st = torch.tensor([COUNTER], dtype=torch.int32, device=dev) if p > 0 else None
            g1, g2 = _nan_grads(q, k1, False), _nan_grads(q, k2, False)

            def run():
                out, lse = ext.attn_fwd2(q, k1, v1, k2, v2, SCALE, ml, p, SEED, st)
                ext.attn_bwd2(q, k1, v1, k2, v2, out, lse, dO, SCALE, g1[1], g1[2], g1[3], g2[2], g2[3], ml, p, SEED, st)
                return out, lse
            (out, lse), got, ndev = profiled(run)
            name = "two_seg.%d" % n
            self.expect(name, {"attn_fwd_narrow_kernel", "attn_bwd_dq_narrow_kernel", "attn_bwd_dkv_kernel<2,0>"}, got, ndev)
            keys = torch.cat([torch.arange(L1), 64 * ((L1 + 63) // 64) + torch.arange(L2)])
            ref = reference(q, torch.cat([k1, k2], 1), torch.cat([v1, v2], 1), SCALE, mk, False, p, SEED,
                            COUNTER if st is not None else None, keys=keys, dO=dO, O_in=out)
            if not (_neighbours_nan(g1[4]) and _neighbours_nan(g2[4][1:])):
                self.fail("%s: a gradient write left its slice" % name)
            self.chk.check_all(name, dict(O=out, lse=lse, dQ=g1[1]), ref, route="two_seg")
            self.chk.check_all(name, dict(dK=torch.cat([g1[2], g2[2]], 1), dV=torch.cat([g1[3], g2[3]], 1)), ref,
                               route="two_seg")

    def probs(self):
        """bq_attn_probs: the map before dropout and the forward's dropped map, elementwise against fp64 P and P^"""
        ext, dev = self.ext, self.dev
        for n, (B, H, Lq, Lk, mask, causal, p) in enumerate([(2, 4, 20, 1045, "m4", False, 0.0), (2, 3, 20, 276, "m9", False, 0.1),
                                                             (2, 3, 37, 37, "m4", True, 0.1), (1, 2, 1, 300, None, False, 0.5)]):
            q, k, v, _, _ = _operands(B, H, Lq, Lk, dev, 970 + n, False)
            mk = _mask(B, Lk, mask, dev, 11) if mask else None
            ml = ext.key_mask_log2(mk.view(B, 1, 1, Lk), B, Lk) if mk is not None else None
            st = torch.tensor([COUNTER], dtype=torch.int32, device=dev) if p > 0 else None
            out, lse = ext.attn_fwd(q, k, v, SCALE, ml, p, SEED, st, causal)
            for pp in ((0.0, p) if p > 0 else (0.0,)):
                P, got, ndev = profiled(lambda: ext.attn_probs(q, k, lse, SCALE, ml, pp, SEED, st, causal))
                name = "probs.%d.p%g" % (n, pp)
                self.expect(name, {"attn_probs_kernel"}, got, ndev)
                self._check_probs(name, P, q, k, lse, mk, causal, pp, st is not None)

    def _check_probs(self, name, P, q, k, lse, mk, causal, p, ctr):
        """P = exp2(c q.k + mask - LSE) of the forward's LSE: the fp64 map P64 within its exponent error (delta, with the
        kernel's LSE as given) -- bound C (delta + 2^-22) P64 with delta as in attn_ref; the dropped map times Z"""
        B, Lq, H, _ = q.shape
        Lk = k.shape[1]
        Q, K = q.double().permute(0, 2, 1, 3), k.double().permute(0, 2, 1, 3)
        s = SCALE * Q @ K.transpose(-1, -2)
        if mk is not None:
            s = s + mk.double().view(B, 1, 1, Lk)
        if causal:
            s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).triu(1), -math.inf)
        lnat = lse.double()[..., None] / 1.4426950408889634
        P64 = torch.exp(s - lnat)
        U = 2.0 ** -24
        delta = 64 * U * SCALE * (Q.abs() @ K.abs().transpose(-1, -2)) + 4 * U * (s.abs() + lnat.abs() + 1.0)
        delta = torch.where(P64 > 0, delta, torch.zeros_like(delta))
        if p > 0:
            P64 = P64 * _keep_mask(SEED, B, H, Lq, Lk, p, q.device, COUNTER if ctr else None).double() / (1.0 - p)
        tol = 3.0 * (delta + 2.0 ** -22) * P64.abs() + 1e-30
        self.chk(name + ".P", P, P64, tol, route="probs")


def battery(dev):
    b = Battery(dev)
    t0 = time.time()
    with torch.no_grad():
        b.extents()
        b.edges()
        b.persist_masks()
        b.pair()
        b.two_segments()
        b.probs()
    torch.cuda.synchronize()
    return b, time.time() - t0


ROUTE_TABLE = ["attn_fwd_narrow_kernel", "attn_fwd_kernel<3,1>", "attn_fwd_kernel<3,0>", "attn_fwd_persist_kernel<3,1>",
               "attn_fwd_persist_kernel<3,0>", "attn_bwd_small_kernel", "attn_bwd_dq_narrow_kernel", "attn_bwd_dq_kernel<4,1>",
               "attn_bwd_dq_kernel<2,0>", "attn_bwd_dkv_kernel<2,1>", "attn_bwd_dkv_kernel<2,0>", "attn_bwd_dq_persist_kernel<3>",
               "attn_bwd_dkv_persist_kernel<2>", "attn_fwd_narrow_pair_kernel", "attn_bwd_dq_narrow_pair_kernel",
               "attn_bwd_dkv_pair_kernel", "attn_probs_kernel"]


def test_kernel_ids_parse_both_name_forms():
    assert kernel_ids(["void bq::attn_fwd_kernel<3, true>(__bf16 const*)", "_ZN2bq15attn_fwd_kernelILi3ELi0EEEvPKDF16b",
                       "_ZN2bq19attn_bwd_dq_kernelILi4ELb1EEEvPKDF16bS2_", "bq::attn_bwd_small_kernel(__bf16 const*)",
                       "attn_bwd_dkv_pair_kernel(bq::AttnPair)", "void at::native::vectorized_elementwise_kernel<4>"]) == {
        "attn_fwd_kernel<3,1>", "attn_fwd_kernel<3,0>", "attn_bwd_dq_kernel<4,1>", "attn_bwd_small_kernel",
        "attn_bwd_dkv_pair_kernel"}


def test_every_attention_route_within_the_fp64_bound(tmp_path):
    out = str(tmp_path / "attn_bound.pt")
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), out], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = p.stdout.decode(errors="replace")
    assert p.returncode == 0, "battery child exited with %d:\n%s" % (p.returncode, log[-6000:])
    r = torch.load(out)
    lines = ["%-28s %.3f" % (k, v) for k, v in sorted(r["ratios"].items())]
    sys.stdout.write("\nattention battery: %d elements held, %.1f s (child %.1f s); largest |err| / bound per route.output:\n%s\n"
                     % (r["checked"], time.time() - t0, r["seconds"], "\n".join(lines)))
    missing = [k for k in ROUTE_TABLE if k not in r["seen"]]
    assert not missing, "route table kernels never launched: %s" % missing
    assert not r["failures"], "%d failures:\n%s" % (len(r["failures"]), "\n".join(r["failures"][:40]))


# ---- repeatability under load -----------------------------------------------------------------------------------------------
def test_resident_grid_kernels_repeatable_under_load(dev):
    from bridgeqa_amd import _ext
    q, k, v, dO, _ = _operands(16, 12, 1025, 1025, dev, 31, False)
    g = torch.empty(16, 1025, 3, 12, 64, device=dev, dtype=torch.bfloat16)

    def fwd_bwd():
        out, lse = _ext.attn_fwd(q, k, v, SCALE)
        _ext.attn_bwd(q, k, v, out, lse, dO, SCALE, g[:, :, 0], g[:, :, 1], g[:, :, 2])
        return out, lse, g
    prev = _ext.attn_set_persistent(7)
    try:
        assert routes(16, 12, 1025, 1025, True, 7, torch.cuda.get_device_properties(dev).multi_processor_count) == \
            profiled(fwd_bwd)[1]
        _repeat_under_load(dev, [fwd_bwd])
    finally:
        _ext.attn_set_persistent(prev)


def test_pair_and_small_kernels_repeatable_under_load(dev):
    from bridgeqa_amd import _ext
    B, H = 3, 4
    st = torch.tensor([COUNTER], dtype=torch.int32, device=dev)
    sides = []
    for s_, Lk in enumerate((1045, 276)):
        q, k, v, dO, _ = _operands(B, H, 20, Lk, dev, 40 + s_, False)
        m = _mask(B, Lk, "m4", dev, Lk)
        _, dq, dk, dv, _ = _nan_grads(q, k, False)
        sides.append(dict(q=q, k=k, v=v, out=torch.empty(B, 20, H, 64, device=dev, dtype=torch.bfloat16),
                          mask_log2=_ext.key_mask_log2(m.view(B, 1, 1, Lk), B, Lk), seed=s_ + 1, grad_out=dO, dq=dq, dk=dk,
                          dv=dv))

    def pair():
        lses = _ext.attn_fwd_pair(sides, SCALE, 0.1, st)
        _ext.attn_bwd_pair([dict(s, lse=l) for s, l in zip(sides, lses)], SCALE, 0.1, st)
        return tuple(lses) + tuple(s[n] for s in sides for n in ("out", "dq", "dk", "dv"))
    q, k, v, dO, _ = _operands(4, 12, 20, 20, dev, 50, False)
    m = _ext.key_mask_log2(_mask(4, 20, "m4", dev, 20).view(4, 1, 1, 20), 4, 20)
    out, lse = _ext.attn_fwd(q, k, v, SCALE, m, 0.1, SEED, st)
    gs = list(_nan_grads(q, k, True)[1:4])

    def small():
        _ext.attn_bwd(q, k, v, out, lse, dO, SCALE, *gs, m, 0.1, SEED, st)
        return tuple(gs)
    assert profiled(small)[1] == {"attn_bwd_small_kernel"}
    _repeat_under_load(dev, [pair, small])


if __name__ == "__main__":
    b, secs = battery(torch.device("cuda:0"))
    torch.save(dict(failures=b.chk.failures, checked=b.chk.checked, ratios=b.chk.ratios, seen=sorted(b.seen), seconds=secs,
                    log=b.log), sys.argv[1])
    print("attention battery: %d elements, %d failures, %.1f s" % (b.chk.checked, len(b.chk.failures), secs))
    for f in b.chk.failures[:40]:
        print("  " + f)
