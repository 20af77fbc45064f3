"""The decode-attention kernels (csrc/attn_decode.hip through _ext.attn_decode_self / attn_decode_cross) held ELEMENTWISE to the
fp64 bound of tests/attn_ref.py.  The reference gets K / V already gathered through the ancestry table by torch; every element of
O must lie inside tolO -- the bound derived for the MFMA kernels with bf16 probabilities: this kernel keeps them in fp32, which
is strictly inside it, so no new tolerance exists here.  Shapes: slot counts that leave a workgroup partly empty (4 waves per
workgroup), one and twelve heads' worth of items, key counts 1, 2, 20 and the edges of the kernel's 32-key chunk."""
import math

import pytest
import torch

from attn_ref import _Checker, reference

pytestmark = pytest.mark.gpu

SCALE = 0.125
NEG = -1e9          # med.py invert_attention_mask


def _chunk():
    from bridgeqa_amd import _ext
    return _ext.DECODE_CHUNK


def _bits(t):
    return t.contiguous().view(torch.int16)


def _self_case(S, H, n, identity, dev, seed):
    """one step at position t = n - 1: returns (qkv, cache, anc, t, gathered K, gathered V)"""
    g = torch.Generator().manual_seed(seed)
    t = n - 1
    Lmax = max(20, n)
    qkv = torch.randn(S, 1, 3, H, 64, generator=g) * 1.5
    qkv[:, :, 2] /= 1.5
    qkv = qkv.to(dev).to(torch.bfloat16)
    cache = torch.randn(S, Lmax, 2, H, 64, generator=g) * 1.5
    cache[:, :, 1] /= 1.5
    cache[:, t:] = math.nan                       # row t is the kernel's to write; rows beyond it must never be read
    cache = cache.to(dev).to(torch.bfloat16)
    if identity:
        anc = torch.arange(S, dtype=torch.int32)[None, :].repeat(Lmax, 1)
    else:
        anc = torch.randint(0, S, (Lmax, S), generator=g, dtype=torch.int32)
    anc = anc.to(dev)
    j = torch.arange(t, device=dev)
    hist = cache[anc[:t].long().t(), j[None, :]]  # (S, t, 2, H, 64): position j of slot s is row anc[j][s]
    K = torch.cat([hist[:, :, 0], qkv[:, :, 1]], dim=1)
    V = torch.cat([hist[:, :, 1], qkv[:, :, 2]], dim=1)
    return qkv, cache, anc, t, K, V


@pytest.mark.parametrize("n", ["1", "2", "20", "c-1", "c", "c+1", "2c+3"])
def test_self_mode_against_the_fp64_bound(dev, n):
    from bridgeqa_amd import _ext
    c = _chunk()
    n = {"1": 1, "2": 2, "20": 20, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+3": 2 * c + 3}[n]
    chk = _Checker()
    total = 0
    for S in (1, 5, 20):
        for H in (2, 12):
            identity = (S, H) == (5, 2)
            qkv, cache, anc, t, K, V = _self_case(S, H, n, identity, dev, seed=1000 * n + 10 * S + H)
            before = cache.clone()
            t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
            calls = _ext.DECODE_CALLS[0]
            # the position from the device counter (the replay route) and from the host value: the same launch
            out = _ext.attn_decode_self(qkv, cache, anc, SCALE, t=0, t_tensor=t_dev)
            after = cache.clone()
            out2 = _ext.attn_decode_self(qkv, cache, anc, SCALE, t=t)
            torch.cuda.synchronize()
            assert _ext.DECODE_CALLS[0] == calls + 2
            name = "self S%d H%d n%d %s" % (S, H, n, "identity" if identity else "random")
            ref = reference(qkv[:, :, 0], K, V, SCALE)
            r = chk(name, out, ref["O"], ref["tolO"])
            total += out.numel()
            print("%-32s max |err| / tol = %.4f" % (name, r))
            assert not torch.isnan(out.float()).any(), name          # the NaN rows beyond t did not leak
            assert torch.equal(_bits(out), _bits(out2)), name         # deterministic; host t == device t
            # row t of the cache is the step's K / V, bit for bit; every other byte is untouched
            assert torch.equal(_bits(after[:, t, 0]), _bits(qkv[:, 0, 1])), name
            assert torch.equal(_bits(after[:, t, 1]), _bits(qkv[:, 0, 2])), name
            keep = torch.ones(cache.shape[1], dtype=torch.bool, device=dev)
            keep[t] = False
            assert torch.equal(_bits(after[:, keep]), _bits(before[:, keep])), name
            assert torch.equal(_bits(cache), _bits(after)), name
    assert not chk.failures, "\n".join(chk.failures)
    assert chk.checked == total                                        # nothing was skipped


def _cross_mask(S, Lk, dev):
    """natural-unit additive key mask (S, Lk): slot 0 (and every slot not named) fully visible, slot 1 ragged, the last slot
    with exactly one visible key; no slot has all keys masked"""
    m = torch.zeros(S, Lk)
    if Lk > 1:
        m[1, max(1, Lk // 2):] = NEG
        m[-1, :] = NEG
        m[-1, Lk // 3] = 0.0
    return m.to(dev)


@pytest.mark.parametrize("Lk", ["1", "7", "35", "c", "c+1"])
def test_cross_mode_against_the_fp64_bound(dev, Lk):
    from bridgeqa_amd import _ext
    c = _chunk()
    Lk = {"1": 1, "7": 7, "35": 35, "c": c, "c+1": c + 1}[Lk]
    chk = _Checker()
    total = 0
    for S, H in ((5, 12), (20, 2), (3, 2)):
        g = torch.Generator().manual_seed(77 * Lk + S + H)
        Xq = (torch.randn(S, 1, 3, H, 64, generator=g) * 1.5).to(dev).to(torch.bfloat16)
        # a block with slack rows and one slack head around it, NaN outside: strided like a HoistedKV block, and a read
        # outside the block shows
        buf = torch.full((S, Lk + 3, 2, H + 1, 64), math.nan)
        inner = torch.randn(S, Lk, 2, H, 64, generator=g) * 1.5
        inner[:, :, 1] /= 1.5
        buf[:, 1:Lk + 1, :, :H] = inner
        buf = buf.to(dev).to(torch.bfloat16)
        kv = buf[:, 1:Lk + 1, :, :H]
        q = Xq[:, :, 0]
        assert not kv.is_contiguous() and not q.is_contiguous()
        for masked in (False, True):
            mask = _cross_mask(S, Lk, dev) if masked else None
            mlog2 = _ext.key_mask_log2(mask[:, None, None, :], S, Lk) if masked else None
            out = _ext.attn_decode_cross(q, kv, SCALE, mlog2)
            out2 = _ext.attn_decode_cross(q, kv, SCALE, mlog2)
            torch.cuda.synchronize()
            name = "cross S%d H%d Lk%d %s" % (S, H, Lk, "masked" if masked else "plain")
            ref = reference(q, kv[:, :, 0], kv[:, :, 1], SCALE, mask=mask)
            r = chk(name, out, ref["O"], ref["tolO"])
            total += out.numel()
            print("%-32s max |err| / tol = %.4f" % (name, r))
            assert torch.equal(_bits(out), _bits(out2)), name
    assert not chk.failures, "\n".join(chk.failures)
    assert chk.checked == total


def test_binding_refuses_what_the_kernel_cannot_address(dev):
    from bridgeqa_amd import _ext
    S, H, L = 2, 2, 4
    qkv = torch.zeros(S, 1, 3, H, 64, dtype=torch.bfloat16, device=dev)
    cache = torch.zeros(S, L, 2, H, 64, dtype=torch.bfloat16, device=dev)
    anc = torch.zeros(L, S, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="position"):
        _ext.attn_decode_self(qkv, cache, anc, SCALE, t=L)
    with pytest.raises(RuntimeError, match="anc"):
        _ext.attn_decode_self(qkv, cache, anc.long(), SCALE, t=0)
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_decode_self(qkv.float(), cache, anc, SCALE, t=0)
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_decode_cross(qkv[:, :, 0], cache[:, :, :, :1], SCALE)     # heads differ
    with pytest.raises(RuntimeError, match="mask_log2"):
        _ext.attn_decode_cross(qkv[:, :, 0], cache, SCALE, torch.zeros(S, L - 1, device=dev))
