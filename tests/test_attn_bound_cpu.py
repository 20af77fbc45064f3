"""The fp64 bound of tests/attn_ref.py proves it can see, on CPU: a CPU emulation of the fused attention kernels' rounding
points (fp32 scores and accumulators, online softmax over 32-key halves of 64-key tiles, bf16 P^ / dS operands, D from the
stored bf16 O, bf16 outputs) passes it with a margin of at least 2 on every element, and nine planted defects -- each
confined to one 32-row wave, one key or one head -- fail it.  The rel-L2 criteria of tests/test_attn_gpu.py (2e-2 on O,
3e-2 on a gradient) are evaluated on each defect and printed, not asserted: they are what this bound replaces."""
import math

import pytest
import torch

from attn_ref import LOG2E, _Checker, _keep_mask, reference

SCALE = 0.125


def _bf(x):
    return x.to(torch.bfloat16).float()


def emulate(q, k, v, scale, mask=None, causal=False, p=0.0, seed=0, counter=None, dO=None, defect=None, wave=None):
    """the kernels' arithmetic in fp32 / bf16: q (B, Lq, H, 64) bf16 etc.; mask natural units (B, Lk).  defect: name of a
    planted bug, applied to wave = (b, h, first row) only (32 rows) unless it names a key or a head"""
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    G = B * H
    f = lambda t: t.float().permute(0, 2, 1, 3).reshape(G, t.shape[1], 64)
    Q, K, V = f(q), f(k), f(v)
    sel = torch.zeros(G, Lq, 1, dtype=torch.bool)
    if wave is not None:
        b, h, r0 = wave
        sel[b * H + h, r0:r0 + 32] = True
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    mk = torch.zeros(G, 1, Lk)
    if mask is not None:
        mk = (mask.float() * torch.tensor(LOG2E, dtype=torch.float32)).reshape(B, 1, 1, Lk).expand(B, H, 1, Lk).reshape(G, 1, Lk)
        if defect == "mask_natural":
            mk = torch.where(sel, mask.float().reshape(B, 1, 1, Lk).expand(B, H, 1, Lk).reshape(G, 1, Lk), mk)
    acc = Q @ K.transpose(1, 2)                                       # fp32 scores (MFMA: fp32 accumulation of bf16 products)
    sc = acc * c + mk
    hide = torch.zeros(G, Lq, Lk, dtype=torch.bool)
    if causal:
        i = torch.arange(Lq).view(Lq, 1)
        j = torch.arange(Lk).view(1, Lk)
        hide = (j > i).expand(G, Lq, Lk).clone()
        if defect == "causal_off":
            hide = torch.where(sel, (j > i + 1).expand(G, Lq, Lk), hide)
    keep = None
    if p > 0:
        keep = _keep_mask(seed, B, H, Lq, Lk, p, "cpu", counter).reshape(G, Lq, Lk)
        if defect == "keep_shift":
            keys = torch.arange(Lk) + 1
            shifted = _keep_mask(seed, B, H, Lq, Lk, p, "cpu", counter, keys=keys).reshape(G, Lq, Lk)
            keep = torch.where(sel, shifted, keep)
    inv_keep = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    sc = sc.masked_fill(hide, -math.inf)
    m = torch.full((G, Lq, 1), -math.inf)
    lsum = torch.zeros(G, Lq, 1)
    o = torch.zeros(G, Lq, 64)
    nkt = (Lk + 63) // 64
    spike_block = None
    for j0 in range(0, Lk, 32):
        blk = slice(j0, min(Lk, j0 + 32))
        s_b = sc[:, :, blk]
        if defect == "skip_tile" and j0 // 64 == nkt - 2:       # one 64-key tile left out of one wave
            s_b = torch.where(sel, torch.full_like(s_b, -math.inf), s_b)
        mnew = torch.maximum(m, s_b.amax(-1, keepdim=True))
        alpha = torch.where(mnew == -math.inf, torch.ones_like(m), torch.exp2(m - mnew))
        m = mnew
        pv = torch.exp2(s_b - torch.where(mnew == -math.inf, torch.zeros_like(mnew), mnew))
        psum = pv.sum(-1, keepdim=True)
        if keep is not None:
            pv = torch.where(keep[:, :, blk], pv * inv_keep, torch.zeros_like(pv))
            if defect == "sum_dropped":
                psum = torch.where(sel, pv.sum(-1, keepdim=True) * (1.0 - p), psum)
        lsum = lsum * alpha + psum
        if defect == "skip_rescale" and spike_block is None and bool(((alpha < 0.5) & sel).any()) and j0 >= Lk // 2:
            spike_block = j0                                    # the late max jump: its rescale of O is skipped
            o = torch.where(sel, o, o * alpha)
        else:
            o = o * alpha
        o = o + _bf(pv) @ V[:, blk]
    O = _bf(o * (1.0 / lsum))
    lse = m[..., 0] + torch.log2(lsum[..., 0])
    res = {"O": O, "lse": lse}
    if defect == "ragged_row":
        res["O"][wave[0] * H + wave[1], Lq - 1] = res["O"][wave[0] * H + wave[1], Lq - 2]
        res["lse"][wave[0] * H + wave[1], Lq - 1] = res["lse"][wave[0] * H + wave[1], Lq - 2]
    if dO is not None:
        Gd = f(dO)
        D = (res["O"] * Gd).sum(-1, keepdim=True)
        if defect == "delta_neighbour":
            D = torch.where(sel, torch.roll(D, -1, 1), D)
        pv = torch.exp2(acc * c + (mk - res["lse"][..., None])).masked_fill(hide, 0.0)
        dP = Gd @ V.transpose(1, 2)
        gv, pd = dP, pv
        if keep is not None:
            gv = torch.where(keep, dP * inv_keep, torch.zeros_like(dP))
            pd = torch.where(keep, pv * inv_keep, torch.zeros_like(pv))
        dS = _bf(pv * (gv - D))
        res["dQ"] = _bf((dS @ K) * scale)
        res["dK"] = _bf((dS.transpose(1, 2) @ Q) * scale)
        res["dV"] = _bf(_bf(pd).transpose(1, 2) @ Gd)
        if defect == "ragged_key":
            g = wave[0] * H + wave[1]
            for n in ("dK", "dV"):
                res[n][g, Lk - 1] = res[n][g, Lk - 2]
        if defect == "swap_dkdv":
            g = wave[0] * H + wave[1]
            res["dK"][g], res["dV"][g] = res["dV"][g].clone(), res["dK"][g].clone()
    for n in list(res):
        t = res[n]
        res[n] = t.reshape(B, H, *t.shape[1:]).permute(0, 2, 1, 3) if t.dim() == 3 else t.reshape(B, H, Lq)
    return res


def _inputs(B, H, Lq, Lk, seed, spike=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, H, 64, generator=g) * 1.5
    k = torch.randn(B, Lk, H, 64, generator=g) * 1.5
    v = torch.randn(B, Lk, H, 64, generator=g)
    dO = torch.randn(B, Lq, H, 64, generator=g)
    if spike is not None:   # a late max jump: one key strongly aligned with the queries of one wave
        b, h, r0, key = spike
        k[b, key, h] = q[b, r0:r0 + 32, h].mean(0) * 6.0
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, dO))


def _mask(B, Lk, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "soft":   # a graded additive bias (relative-position style), natural units
        return -3.0 * torch.rand(B, Lk, generator=g)
    big = -10000.0 if kind == "m4" else -1e9
    m = torch.zeros(B, Lk)
    m[0, Lk // 2:] = big
    if B > 1:
        m[1, 1:] = big            # one sample with a single unmasked key
    return m


CLEAN = [  # B, H, Lq, Lk, mask, causal, p, counter, spike
    (1, 2, 33, 33, None, False, 0.0, None, None),
    (1, 2, 129, 129, None, False, 0.0, None, (0, 1, 64, 120)),
    (2, 2, 70, 200, "m4", False, 0.0, None, None),
    (2, 2, 20, 161, "m9", False, 0.1, 7, None),
    (1, 2, 130, 97, "soft", False, 0.5, None, None),
    (1, 2, 257, 257, None, True, 0.0, None, None),
    (2, 1, 129, 129, "m4", True, 0.1, 3, None),
    (1, 1, 1, 65, None, False, 0.0, None, None),
]


@pytest.mark.parametrize("B,H,Lq,Lk,mask,causal,p,counter,spike", CLEAN)
def test_kernel_rounding_emulation_passes_with_margin(B, H, Lq, Lk, mask, causal, p, counter, spike):
    q, k, v, dO = _inputs(B, H, Lq, Lk, Lq * 31 + Lk, spike)
    mk = _mask(B, Lk, mask, Lk) if mask else None
    emu = emulate(q, k, v, SCALE, mk, causal, p, 99, counter, dO)
    ref = reference(q, k, v, SCALE, mk, causal, p, 99, counter, dO=dO, O_in=emu["O"].to(torch.bfloat16))
    chk = _Checker()
    chk.check_all("emu", emu, ref)
    assert not chk.failures, "\n".join(chk.failures)
    worst = max(chk.ratios.values())
    assert worst <= 0.5, ("margin below 2", chk.ratios)
    assert chk.checked > 0


# name, shape (B, H, Lq, Lk), mask kind, causal, p, wave (b, h, first row), spike
DEFECTS = [
    ("skip_tile", (1, 2, 256, 256), None, False, 0.0, (0, 1, 96), None),
    ("skip_rescale", (1, 2, 256, 256), None, False, 0.0, (0, 1, 64), (0, 1, 64, 230)),
    ("sum_dropped", (1, 2, 256, 256), None, False, 0.1, (0, 1, 32), None),
    ("keep_shift", (1, 2, 256, 256), None, False, 0.1, (0, 0, 160), None),
    ("delta_neighbour", (1, 2, 256, 256), None, False, 0.0, (0, 1, 128), None),
    ("ragged_row", (1, 2, 257, 257), None, False, 0.0, (0, 1, 256), None),
    ("ragged_key", (1, 2, 257, 257), None, False, 0.0, (0, 0, 256), None),
    ("causal_off", (1, 2, 256, 256), None, True, 0.0, (0, 1, 0), None),
    ("mask_natural", (1, 2, 256, 256), "soft", False, 0.0, (0, 0, 224), None),
    ("swap_dkdv", (1, 2, 256, 256), None, False, 0.0, (0, 1, 0), None),
]


@pytest.mark.parametrize("name,shape,mask,causal,p,wave,spike", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_fails_the_bound(name, shape, mask, causal, p, wave, spike):
    B, H, Lq, Lk = shape
    q, k, v, dO = _inputs(B, H, Lq, Lk, 5 + Lq, spike)
    mk = _mask(B, Lk, mask, 3) if mask else None
    good = emulate(q, k, v, SCALE, mk, causal, p, 1234, 5, dO)
    bad = emulate(q, k, v, SCALE, mk, causal, p, 1234, 5, dO, defect=name, wave=wave)
    changed = [n for n in good if not torch.equal(good[n], bad[n])]
    assert changed, "the defect changed nothing"
    ref = reference(q, k, v, SCALE, mk, causal, p, 1234, 5, dO=dO, O_in=bad["O"].to(torch.bfloat16))
    chk = _Checker()
    chk.check_all(name, bad, ref)
    assert chk.failures, "planted defect %s passed the fp64 bound" % name
    # what the whole-tensor criteria of tests/test_attn_gpu.py would have said (reported, not asserted)
    rel = lambda n: float((bad[n].double() - ref[n]).norm() / ref[n].norm())
    lims = {"O": 2e-2, "dQ": 3e-2, "dK": 3e-2, "dV": 3e-2}
    vit = math.sqrt(bad["O"].numel() / (16 * 1025 * 12 * 64))   # the same error inside a (16, 12, 1025) tensor
    seen = [n for n in lims if rel(n) >= lims[n]]
    seen_vit = [n for n in lims if rel(n) * vit >= lims[n]]
    print("\n%s: rel-L2 %s -> here %s, inside (16, 12, 1025) %s" % (
        name, ", ".join("%s %.2e" % (n, rel(n)) for n in lims), ",".join(seen) or "MISSED", ",".join(seen_vit) or "MISSED"))
