"""The candidate-attention entry points of answer ranking (csrc/attn_rank.hip: bq_attn_rank_self / bq_attn_rank_cross) as far
as they can be checked without a GPU: the ABI surface, the argument checks (nothing is launched: the checks come first), the
CPU / dtype / mask rejection of the bindings, and the kernels' compile-time footprint (no LDS, no scratch)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("bq_attn_rank_self", "bq_attn_rank_cross")
EINVAL, ELIMIT = -1, -2


def test_header_declares_and_library_exports_the_rank_entry_points():
    from bridgeqa_amd import _ext
    hdr = open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    syms = set(re.findall(r"BQ_API\s+int\s+(bq_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(_ext.library_path())
    for s in ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
    assert lib.bq_abi_version() == 6          # the addition is purely additive
    assert int(re.search(r"#define BQ_RANK_LMAX (\d+)", hdr).group(1)) == _ext.RANK_LMAX
    assert int(re.search(r"#define BQ_RANK_QBLOCK (\d+)", hdr).group(1)) == _ext.RANK_QBLOCK
    assert _ext.RANK_QBLOCK in (4, 8) and len(_ext.RANK_CALLS) == 2


# the argument tails of a healthy call: N = 6 sequences of La = 5 tokens, 12 heads, packed (N, La, 3, H, 64) / (N, La, H, 64)
# operands, 2 questions x 3 candidates over a (2, 7, 2, H, 64) block
SELF_STRIDES = (5 * 2304, 2304, 768, 64) + (5 * 768, 768, 64)
CROSS_STRIDES = (5 * 768, 768, 64) + (7 * 1536, 1536, 64) + (5 * 768, 768, 64)


def _self(lib, qkv, O, mask, N=6, H=12, La=5, Lap=64, strides=SELF_STRIDES):
    return lib.bq_attn_rank_self(qkv, O, mask, N, H, La, Lap, *strides, 0.125, None)


def _cross(lib, Q, K, V, O, mask, N=6, Bq=2, group=3, H=12, La=5, Lk=7, Lkp=64, strides=CROSS_STRIDES):
    return lib.bq_attn_rank_cross(Q, K, V, O, mask, N, Bq, group, H, La, Lk, Lkp, *strides, 0.125, None)


def test_bad_arguments_are_refused_with_the_entrys_name_and_nothing_is_launched():
    from bridgeqa_amd import _ext
    lib = _ext._lib
    buf = torch.zeros(64, dtype=torch.bfloat16)      # a real, 16-byte aligned host pointer: no check may dereference it
    p = buf.data_ptr()
    assert p % 16 == 0

    def refused(code, status, entry, word=None):
        assert status == code, (status, lib.bq_last_error())
        err = lib.bq_last_error()
        assert entry in err, err
        assert word is None or word in err, err

    # null pointers
    refused(EINVAL, _self(lib, None, None, None), b"attn_rank_self", b"null")
    refused(EINVAL, _self(lib, p, None, None), b"attn_rank_self")
    refused(EINVAL, _cross(lib, None, None, None, None, None), b"attn_rank_cross", b"null")
    refused(EINVAL, _cross(lib, p, p, None, p, None), b"attn_rank_cross")
    # no sequences: a no-op success, whatever else is passed; a negative count is not
    assert _self(lib, None, None, None, N=0) == 0
    assert _cross(lib, None, None, None, None, None, N=0, Bq=0) == 0
    refused(EINVAL, _self(lib, p, p, None, N=-1), b"attn_rank_self")
    refused(EINVAL, _cross(lib, p, p, p, p, None, N=-1), b"attn_rank_cross")
    # the self form holds RANK_LMAX tokens in registers
    lmax = _ext.RANK_LMAX
    refused(ELIMIT, _self(lib, p, p, None, La=lmax + 1, Lap=0), b"attn_rank_self", str(lmax).encode())
    # N is not Bq x group
    refused(EINVAL, _cross(lib, p, p, p, p, None, N=7), b"attn_rank_cross", b"candidates")
    refused(EINVAL, _cross(lib, p, p, p, p, None, N=6, Bq=2, group=4), b"attn_rank_cross", b"candidates")
    refused(EINVAL, _cross(lib, p, p, p, p, None, N=6, Bq=6, group=0), b"attn_rank_cross")
    # a mask narrower than the keys
    refused(EINVAL, _cross(lib, p, p, p, p, p, Lk=7, Lkp=6), b"attn_rank_cross")
    refused(EINVAL, _self(lib, p, p, p, La=5, Lap=4), b"attn_rank_self")
    # strides that are no multiple of 8 elements, pointers off a 16-byte boundary
    for k in range(len(SELF_STRIDES)):
        s = list(SELF_STRIDES)
        s[k] += 4
        refused(EINVAL, _self(lib, p, p, None, strides=s), b"attn_rank_self", b"aligned")
    for k in range(len(CROSS_STRIDES)):
        s = list(CROSS_STRIDES)
        s[k] += 4
        refused(EINVAL, _cross(lib, p, p, p, p, None, strides=s), b"attn_rank_cross", b"aligned")
    refused(EINVAL, _self(lib, p + 8, p, None), b"attn_rank_self", b"aligned")
    refused(EINVAL, _cross(lib, p, p + 8, p, p, None), b"attn_rank_cross", b"aligned")


def test_bindings_refuse_host_tensors_wrong_dtypes_and_wrong_masks():
    from bridgeqa_amd import _ext
    N, H, La, Lk = 6, 2, 3, 5
    qkv = torch.zeros(N, La, 3, H, 64, dtype=torch.bfloat16)
    kv = torch.zeros(2, Lk, 2, H, 64, dtype=torch.bfloat16)
    calls = list(_ext.RANK_CALLS)
    with pytest.raises(RuntimeError, match="attn_rank_self: qkv: CPU not supported"):
        _ext.attn_rank_self(qkv, 0.125)
    with pytest.raises(RuntimeError, match="attn_rank_cross: q: CPU not supported"):
        _ext.attn_rank_cross(qkv[:, :, 0], kv, 0.125, 3)
    # the operand checks themselves need no device: a stand-in that only claims to be a CUDA tensor reaches them
    class _Dev(object):
        """the attributes the checks read, with is_cuda set: shape / dtype / stride checks run before any launch"""
        def __init__(self, t):
            self.t = t
        is_cuda = True

        def __getattr__(self, n):
            return getattr(self.t, n)
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_rank_self(_Dev(qkv.float()), 0.125)
    with pytest.raises(RuntimeError, match="bf16"):
        _ext.attn_rank_cross(_Dev(qkv[:, :, 0]), _Dev(kv.float()), 0.125, 3)
    with pytest.raises(RuntimeError, match="holds %d" % _ext.RANK_LMAX):
        _ext.attn_rank_self(_Dev(torch.zeros(1, _ext.RANK_LMAX + 1, 3, H, 64, dtype=torch.bfloat16)), 0.125)
    with pytest.raises(RuntimeError, match="mask_log2"):
        _ext.attn_rank_self(_Dev(qkv), 0.125, _Dev(torch.zeros(N, La - 1)))
    with pytest.raises(RuntimeError, match="mask_log2"):
        _ext.attn_rank_cross(_Dev(qkv[:, :, 0]), _Dev(kv), 0.125, 3, _Dev(torch.zeros(N, 64)))
    with pytest.raises(RuntimeError, match="group"):
        _ext.attn_rank_cross(_Dev(qkv[:, :, 0]), _Dev(kv), 0.125, 4)
    assert _ext.RANK_CALLS == calls


def test_rank_kernels_use_no_lds_and_no_scratch():
    from bridgeqa_amd import build
    build.build()
    res = build.kernel_resources()
    if res is None:
        pytest.skip("objects were not compiled by this checkout's build.py (prebuilt library)")
    mine = {k: v for k, v in res.items() if "attn_rank" in k}
    assert len(mine) == 2, sorted(mine)
    for k, v in mine.items():
        assert v.get("lds", 0) == 0, (k, v)
        assert v.get("scratch", 0) == 0, (k, v)
