"""The candidate-attention kernels of answer ranking (csrc/attn_rank.hip through _ext.attn_rank_self / attn_rank_cross) held
ELEMENTWISE to the fp64 bound of tests/attn_ref.py, exactly as tests/test_attn_decode_gpu.py holds the decode kernels: every
element of O must lie inside tolO -- the bound derived for the MFMA kernels with bf16 probabilities; these kernels keep them in
fp32, which is strictly inside it, so no new tolerance exists here.  The cross form's reference gets K / V repeated per sequence
by torch.  Shapes: sequence counts that leave a workgroup partly empty (4 waves per workgroup), 2 and 12 heads, sequence lengths
1, 2, 5 and the edges of RANK_LMAX, query counts around RANK_QBLOCK, key counts 1, 7, 35 and the edges of the 32-key chunk."""
import math

import pytest
import torch

from attn_ref import _Checker, reference

pytestmark = pytest.mark.gpu

SCALE = 0.125
NEG_SELF = -10000.0     # med.py get_extended_attention_mask
NEG = -1e9              # med.py invert_attention_mask


def _consts():
    from bridgeqa_amd import _ext
    return _ext.RANK_LMAX, _ext.RANK_QBLOCK


def _bits(t):
    return t.contiguous().view(torch.int16)


def _self_mask(N, La, kind, dev):
    """natural-unit additive key mask (N, La): 'ragged' -- sequence s keeps its first 1 + (3 s + 1) % La tokens (pad tails of
    different lengths, sequence 0 often whole); 'first' -- as ragged, but the last sequence sees token 0 only"""
    if kind == "none":
        return None
    m = torch.zeros(N, La)
    for s in range(N):
        m[s, 1 + (3 * s + 1) % La:] = NEG_SELF
    if kind == "first":
        m[-1, 1:] = NEG_SELF
    return m.to(dev)


@pytest.mark.parametrize("La", ["1", "2", "5", "max-1", "max"])
def test_self_form_against_the_fp64_bound(dev, La):
    from bridgeqa_amd import _ext
    lmax, _ = _consts()
    La = {"1": 1, "2": 2, "5": 5, "max-1": lmax - 1, "max": lmax}[La]
    chk = _Checker()
    total = launches = 0
    calls = list(_ext.RANK_CALLS)
    for N in (1, 5, 20):
        for H in (2, 12):
            g = torch.Generator().manual_seed(1000 * La + 10 * N + H)
            # the packed projection as a strided slice of a larger NaN-filled buffer: slack rows before and after every sequence
            # and one slack head, so a read outside the sequence's rows or heads shows in the output
            buf = torch.full((N, La + 2, 3, H + 1, 64), math.nan)
            inner = torch.randn(N, La, 3, H, 64, generator=g) * 1.5
            inner[:, :, 2] /= 1.5
            buf[:, 1:La + 1, :, :H] = inner
            buf = buf.to(dev).to(torch.bfloat16)
            qkv = buf[:, 1:La + 1, :, :H]
            assert not qkv.is_contiguous()
            for kind in ("none", "ragged", "first"):
                mask = _self_mask(N, La, kind, dev)
                mlog2 = _ext.key_mask_log2(mask[:, None, None, :], N, La) if mask is not None else None
                out = _ext.attn_rank_self(qkv, SCALE, mlog2)
                out2 = _ext.attn_rank_self(qkv, SCALE, mlog2)
                torch.cuda.synchronize()
                launches += 2
                name = "self N%d H%d La%d %s" % (N, H, La, kind)
                ref = reference(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], SCALE, mask=mask, causal=True)
                r = chk(name, out, ref["O"], ref["tolO"])
                total += out.numel()
                print("%-32s max |err| / tol = %.4f" % (name, r))
                assert tuple(out.shape) == (N, La, H, 64) and out.dtype == torch.bfloat16
                assert not torch.isnan(out.float()).any(), name          # nothing outside the sequence was read
                assert torch.equal(_bits(out), _bits(out2)), name         # bitwise reproducible
    assert _ext.RANK_CALLS == [calls[0] + launches, calls[1]]
    assert not chk.failures, "\n".join(chk.failures)
    assert chk.checked == total                                            # nothing was skipped


def _cross_mask(Bq, Lk, kind, dev):
    """natural-unit additive key mask (Bq, Lk): question 0 fully visible, question 1 (when there is one) ragged; 'single' -- the
    last question with exactly one visible key.  No question has all keys masked."""
    if kind == "none":
        return None
    m = torch.zeros(Bq, Lk)
    if Lk > 1:
        if Bq > 1:
            m[1, max(1, Lk // 2):] = NEG
        if kind == "single":
            m[-1, :] = NEG
            m[-1, Lk // 3] = 0.0
    return m.to(dev)


@pytest.mark.parametrize("Lk", ["1", "7", "35", "32", "33"])
def test_cross_form_against_the_fp64_bound(dev, Lk):
    from bridgeqa_amd import _ext
    _, qb = _consts()
    Lk = int(Lk)
    chk = _Checker()
    total = launches = 0
    calls = list(_ext.RANK_CALLS)
    las = (1, qb - 1, qb, qb + 1, 2 * qb + 1)
    cases = [(bq, group, H) for bq in (1, 3) for group in (1, 3, 4) for H in ((12,) if (bq, group) == (3, 4) else (2,))]
    for n_case, (Bq, group, H) in enumerate(cases):
        N = Bq * group
        for La in las:
            g = torch.Generator().manual_seed(77 * Lk + 13 * N + 5 * La + H)
            Xq = (torch.randn(N, La, 3, H, 64, generator=g) * 1.5).to(dev).to(torch.bfloat16)
            q = Xq[:, :, 0]                                  # strided: the query third of a packed buffer
            # K / V as a strided slice of a NaN-padded block: a HoistedKV block with slack rows and a slack head
            buf = torch.full((Bq, Lk + 3, 2, H + 1, 64), math.nan)
            inner = torch.randn(Bq, Lk, 2, H, 64, generator=g) * 1.5
            inner[:, :, 1] /= 1.5
            buf[:, 1:Lk + 1, :, :H] = inner
            buf = buf.to(dev).to(torch.bfloat16)
            kv = buf[:, 1:Lk + 1, :, :H]
            assert not kv.is_contiguous() and (N * La == 1 or not q.is_contiguous())
            rep = kv.repeat_interleave(group, dim=0)        # what the reference composition tiles: K / V of sequence n
            for kind in ("none", "ragged", "single"):
                mask = _cross_mask(Bq, Lk, kind, dev)
                mlog2 = _ext.key_mask_log2(mask[:, None, None, :], Bq, Lk) if mask is not None else None
                out = _ext.attn_rank_cross(q, kv, SCALE, group, mlog2)
                out2 = _ext.attn_rank_cross(q, kv, SCALE, group, mlog2)
                torch.cuda.synchronize()
                launches += 2
                name = "cross Bq%d g%d H%d La%d Lk%d %s" % (Bq, group, H, La, Lk, kind)
                ref = reference(q, rep[:, :, 0], rep[:, :, 1], SCALE,
                                mask=mask.repeat_interleave(group, dim=0) if mask is not None else None)
                r = chk(name, out, ref["O"], ref["tolO"])
                total += out.numel()
                print("%-40s max |err| / tol = %.4f" % (name, r))
                assert tuple(out.shape) == (N, La, H, 64) and out.dtype == torch.bfloat16
                assert not torch.isnan(out.float()).any(), name
                assert torch.equal(_bits(out), _bits(out2)), name
    assert _ext.RANK_CALLS == [calls[0], calls[1] + launches]
    assert not chk.failures, "\n".join(chk.failures)
    assert chk.checked == total


def test_binding_refuses_what_the_kernels_cannot_address(dev):
    from bridgeqa_amd import _ext
    lmax, _ = _consts()
    N, H, La, Lk = 6, 2, 3, 5
    qkv = torch.zeros(N, La, 3, H, 64, dtype=torch.bfloat16, device=dev)
    kv = torch.zeros(2, Lk, 2, H, 64, dtype=torch.bfloat16, device=dev)
    calls = list(_ext.RANK_CALLS)
    with pytest.raises(RuntimeError, match="holds %d" % lmax):
        _ext.attn_rank_self(torch.zeros(1, lmax + 1, 3, H, 64, dtype=torch.bfloat16, device=dev), SCALE)
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_rank_self(qkv.float(), SCALE)
    with pytest.raises(RuntimeError, match="mask_log2"):
        _ext.attn_rank_self(qkv, SCALE, torch.zeros(N, La - 1, device=dev))
    with pytest.raises(RuntimeError, match="group"):
        _ext.attn_rank_cross(qkv[:, :, 0], kv, SCALE, 4)                    # 6 sequences are not 2 questions x 4
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_rank_cross(qkv[:, :, 0], kv[:, :, :, :1], SCALE, 3)       # heads differ
    with pytest.raises(RuntimeError, match="mask_log2"):
        _ext.attn_rank_cross(qkv[:, :, 0], kv, SCALE, 3, torch.zeros(N, 64, device=dev))   # a mask per sequence, not per question
    with pytest.raises(RuntimeError, match="strides"):
        _ext.attn_rank_cross(qkv[:, :, 0], torch.zeros(2, Lk, 2, H, 68, dtype=torch.bfloat16, device=dev)[..., 4:], SCALE, 3)
    assert _ext.RANK_CALLS == calls                                          # nothing was launched
