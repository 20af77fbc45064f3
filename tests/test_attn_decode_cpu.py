"""The decode-attention entry points (csrc/attn_decode.hip: bq_attn_decode_self / bq_attn_decode_cross) and the ancestry table
of ops.DecodeCache, as far as they can be checked without a GPU: the ABI surface and its argument checks, the CPU rejection
of the bindings, the table update against a physical reorder of the cache, and the kernels' compile-time footprint."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("bq_attn_decode_self", "bq_attn_decode_cross")


def test_header_declares_and_library_exports_the_decode_entry_points():
    from bridgeqa_amd import _ext
    hdr = open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    syms = set(re.findall(r"BQ_API\s+int\s+(bq_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(_ext.library_path())
    for s in ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
    assert lib.bq_abi_version() == 6          # the addition is purely additive


def test_null_pointers_and_bad_extents_are_refused_and_zero_slots_is_a_no_op():
    from bridgeqa_amd import _ext
    lib = _ext._lib
    self_tail = (5, 12, 20) + (2304, 768, 64) + (30720 * 2, 1536, 768, 64) + (768, 64)
    assert lib.bq_attn_decode_self(None, None, None, None, None, 0, *self_tail, 0.125, None) == -1
    assert b"attn_decode_self" in lib.bq_last_error()
    assert lib.bq_attn_decode_self(None, None, None, None, None, 0, -1, 12, 20, *self_tail[3:], 0.125, None) == -1
    assert lib.bq_attn_decode_self(None, None, None, None, None, 0, 0, 12, 20, *self_tail[3:], 0.125, None) == 0
    cross_tail = (5, 12, 7, 64) + (768, 64) + (7 * 1536, 1536, 64) + (768, 64)
    assert lib.bq_attn_decode_cross(None, None, None, None, None, *cross_tail, 0.125, None) == -1
    assert b"attn_decode_cross" in lib.bq_last_error()
    assert lib.bq_attn_decode_cross(None, None, None, None, None, 5, 0, 7, 64, *cross_tail[4:], 0.125, None) == -1
    assert lib.bq_attn_decode_cross(None, None, None, None, None, 0, 12, 7, 64, *cross_tail[4:], 0.125, None) == 0
    # a real pointer does not rescue non-positive extents (nothing is launched: the checks come first)
    buf = torch.zeros(64, dtype=torch.bfloat16)
    p = buf.data_ptr()
    assert lib.bq_attn_decode_cross(p, p, p, p, None, 1, 1, 0, 0, 64, 64, 64, 64, 64, 64, 64, 0.125, None) == -1
    assert lib.bq_attn_decode_self(p, p, p, p, None, 3, 1, 1, 2, 192, 64, 64, 256, 128, 64, 64, 64, 64, 0.125, None) == -1
    assert b"position" in lib.bq_last_error()


def test_host_tensors_are_rejected():
    from bridgeqa_amd import _ext
    S, H, L = 2, 2, 4
    qkv = torch.zeros(S, 1, 3, H, 64, dtype=torch.bfloat16)
    cache = torch.zeros(S, L, 2, H, 64, dtype=torch.bfloat16)
    anc = torch.zeros(L, S, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attn_decode_self(qkv, cache, anc, 0.125, t=0)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attn_decode_cross(qkv[:, :, 0], cache, 0.125)


def _schedule(B, K, gen):
    """five beam_idx vectors as generation.beam_search lines 104-106 leave them: per sample a choice of source beams with
    duplicates (so others are dropped), and the identity (base + arange) for a sample that has finished"""
    base = (torch.arange(B) * K).unsqueeze(1)
    out = []
    for step in range(5):
        pick = torch.randint(0, K, (B, K), generator=gen)
        pick[:, 1] = pick[:, 0]                               # a duplicate in every sample
        idx = pick + base
        if step >= 2:                                          # sample 1 is done from the third step on
            idx[1] = base[1] + torch.arange(K)
        if step == 3:
            idx[0] = base[0] + torch.arange(K).flip(0)         # a pure permutation
        out.append(idx.reshape(-1))
    return out


def test_ancestry_table_equals_a_physical_reorder_of_the_cache():
    """after every step the history gathered through anc is, bit for bit, what index_select-ing the whole cache (the reference's
    _reorder_cache, models/med.py:1466-1470) leaves in its rows"""
    from bridgeqa_amd import fusion_ops as ops
    gen = torch.Generator().manual_seed(11)
    B, K, Lmax = 3, 4, 8
    S = B * K
    static = torch.zeros(S, Lmax, 2, 3, dtype=torch.float32)      # stays in place, read through anc
    anc = torch.arange(S, dtype=torch.int32)[None, :].repeat(Lmax, 1)
    physical = torch.zeros(S, 0, 2, 3)                            # grows and is reordered, as today's cache
    t = 0
    for beam_idx in _schedule(B, K, gen):
        row = torch.randn(S, 2, 3, generator=gen)                 # the step's K / V rows: slot s writes [s, t]
        static[:, t] = row
        physical = torch.cat([physical, row[:, None]], dim=1)
        t += 1                                                    # DecodeCache.advance
        ops.reorder_ancestry(anc, t, beam_idx)                    # DecodeCache.reorder
        physical = physical.index_select(0, beam_idx)
        hist = ops.gather_history(static, anc, t)
        assert hist.shape == physical.shape
        assert torch.equal(hist, physical), t
        assert torch.equal(anc[t], torch.arange(S, dtype=torch.int32))
        assert torch.equal(anc[t + 1:], torch.arange(S, dtype=torch.int32)[None, :].repeat(Lmax - t - 1, 1))
    # the last reorder of a decode that filled the cache has no row t to reset
    full = torch.arange(S, dtype=torch.int32)[None, :].repeat(2, 1)
    ops.reorder_ancestry(full, 2, torch.arange(S).flip(0))
    assert torch.equal(full[0].long(), torch.arange(S).flip(0))


def test_decode_kernels_use_no_scratch():
    from bridgeqa_amd import build
    build.build()
    res = build.kernel_resources()
    if res is None:
        pytest.skip("objects were not compiled by this checkout's build.py (prebuilt library)")
    mine = {k: v for k, v in res.items() if "attn_decode" in k}
    assert len(mine) >= 2, sorted(mine)
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0, (k, v)
