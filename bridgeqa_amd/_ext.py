"""`pointnet2._ext` for MI355X: the reference's nine-function operator surface
(lib/pointnet2/_ext_src/src/bindings.cpp:6-19) bound to libbqhip.so through ctypes.

What the reference's C++ wrappers do on the host is done here: dtype / contiguity / device checks
(include/utils.h:5-25), output allocation (zero-filled where the kernel accumulates), and turning
a non-zero status into a Python exception (the reference prints and exit(-1)s instead).
There is NO CPU path: like the reference ("CPU not supported", sampling.cpp:34) a host tensor
raises, and a missing library raises at import time.
"""
import ctypes
import os

import torch  # must be imported first: libbqhip.so resolves libamdhip64.so.7 to torch's copy

from . import _cabi, gemm_route
from .gemm_route import GEMM_TILE_ROWS, TILE256_MIN_K, pick_tile  # noqa: F401  (the GEMM tile policy; tools flip these by name)

# (BQHIP_LIB: another build of the same sources, e.g. with a measurement macro set -- A/B runs in one gpurun call)
_LIB_PATH = os.environ.get("BQHIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libbqhip.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        "bridgeqa_amd: %s is missing -- build it with `python -m bridgeqa_amd.build` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback." % _LIB_PATH)

_lib = ctypes.CDLL(_LIB_PATH)
# Every prototype, descriptor struct and integer constant below comes from include/bqhip.h and include/bqhip_fusion.h (_cabi.py).
_D = _cabi.DEFINES
_cabi.bind(_lib, ("bq_abi_version", "bq_last_error"))
ABI_VERSION = _D["BQHIP_ABI_VERSION"]
if _lib.bq_abi_version() != ABI_VERSION:
    raise ImportError("bridgeqa_amd: libbqhip.so ABI %d != %d (stale library: python -m bridgeqa_amd.build --force)"
                      % (_lib.bq_abi_version(), ABI_VERSION))
_cabi.bind(_lib)
_cabi.bind(_lib, _cabi.ADDITIVE_PROTOS)
_cabi.bind(_lib, _cabi.EXTENSION_PROTOS)
_cabi.bind(_lib, _cabi.MCAN_PROTOS)
_cabi.bind(_lib, _cabi.MHATT_PROTOS)

# ---- the deterministic training mode (bridgeqa_amd.set_deterministic) ------------------------------------------------------------
# Every site of the training path where float atomics from several workgroups met on one address, the entry point that takes it in
# the deterministic mode and the kernels that entry launches (none holds a float atomic: tests/test_deterministic_cpu.py reads their
# ISA).  The dispatchers below call the entry named here.  Single adders onto a value an earlier launch stored (gemm `accum`, the
# second row source of a weight gradient) were already reproducible; they run on gemm64_kernel_det too.
DET_ROUTES = {
    "ln_bwd": dict(entry="bq_drop_add_ln_bwd_det", src="ln.hip",
                   kernels=("drop_add_ln_bwd_kernel_det", "ln_dgb_fold_det_kernel")),
    "colsum_grouped": dict(entry="bq_colsum_grouped_det_bf16", src="gemm.hip",
                           kernels=("colsum_grouped_det_kernel", "colsum_grouped_fold_det_kernel")),
    # fp32-output small-tile GEMMs: cut contractions (the LM head's dH) into per-piece slabs, accum with plain stores
    "gemm_splitk_f32": dict(entry="bq_gemm_bf16", src="gemm.hip", kernels=("gemm64_kernel_det",)),
    "gemm_splitk_fold": dict(entry="bq_gemm_splitk_fold_det", src="gemm.hip", kernels=("splitk_fold_det_kernel",)),
    # column sums in a bf16-output GEMM epilogue: the GEMM runs without them, the grouped fixed-order column sum takes them
    "gemm_epilogue_colsum": dict(entry="bq_colsum_grouped_det_bf16", src="gemm.hip",
                                 kernels=("colsum_grouped_det_kernel", "colsum_grouped_fold_det_kernel")),
}


def _det():
    from . import is_deterministic
    return is_deterministic()


def _det_entry(site):
    return getattr(_lib, DET_ROUTES[site]["entry"])


def _ln_bwd_det(x, residual, gamma, gamma2, groups, dy, dsum, mean, rstd, dx, dres, dgb, M, H, eps, p_drop, p_path,
                rows_per_sample, seed, seed_tensor, x_is_sum, what):
    slab = torch.empty(max(1, _lib.bq_drop_add_ln_bwd_det_slab_floats(M, H, groups)), dtype=torch.float32, device=x.device)
    _check(_det_entry("ln_bwd")(_p(x), _p(residual), _p(gamma), _p(gamma2), groups, _p(dy), _p(dsum), _p(mean), _p(rstd),
                                _p(dx), _p(dres), _p(dgb), _p(slab), M, H, float(eps), float(p_drop), float(p_path),
                                int(rows_per_sample), int(seed) & 0xFFFFFFFF, _p(seed_tensor), int(x_is_sum), _stream()), what)


def library_path():
    return _LIB_PATH


def _check(status, what):
    if status != 0:
        raise RuntimeError("%s failed (status %d): %s" % (what, status, _lib.bq_last_error().decode()))


def _req(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported (bridgeqa_amd has no CPU path)" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be a %s tensor" % (name, "float" if dtype == torch.float32 else "int"))


def _same_device(*ts):
    d = ts[0].device
    for t in ts[1:]:
        if t.device != d:
            raise RuntimeError("all tensors must be on the same device")


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def opt_n_threads(n):
    return _lib.bq_opt_n_threads(int(n))


def furthest_point_sampling(points, nsamples):
    _req(points, torch.float32, "points")
    B, N, _ = points.shape
    with torch.cuda.device(points.device):
        out = torch.zeros(B, nsamples, dtype=torch.int32, device=points.device)
        nbytes = _lib.bq_fps_workspace_bytes(B, N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device) if nbytes else None
        _check(_lib.bq_furthest_point_sampling(_p(points), _p(ws), nbytes, _p(out), B, N, int(nsamples), _stream()),
               "furthest_point_sampling")
    return out


def furthest_point_sampling_bruteforce(points, nsamples):
    """Unpruned kernels (A/B timing, independent cross-check of the bucketed kernel)."""
    _req(points, torch.float32, "points")
    B, N, _ = points.shape
    with torch.cuda.device(points.device):
        out = torch.zeros(B, nsamples, dtype=torch.int32, device=points.device)
        tmp = torch.empty(B, N, dtype=torch.float32, device=points.device) if N > 24576 else None
        _check(_lib.bq_furthest_point_sampling_bruteforce(_p(points), _p(tmp), _p(out), B, N, int(nsamples),
                                                          _stream()), "furthest_point_sampling_bruteforce")
    return out


def gather_points(points, idx):
    _req(points, torch.float32, "points"); _req(idx, torch.int32, "idx"); _same_device(points, idx)
    B, C, N = points.shape
    M = idx.shape[1]
    with torch.cuda.device(points.device):
        out = torch.empty(B, C, M, dtype=torch.float32, device=points.device)
        _check(_lib.bq_gather_points(_p(points), _p(idx), _p(out), B, C, N, M, _stream()), "gather_points")
    return out


def gather_points_grad(grad_out, idx, n):
    _req(grad_out, torch.float32, "grad_out"); _req(idx, torch.int32, "idx"); _same_device(grad_out, idx)
    B, C, M = grad_out.shape
    with torch.cuda.device(grad_out.device):
        out = torch.zeros(B, C, n, dtype=torch.float32, device=grad_out.device)
        _check(_lib.bq_gather_points_grad(_p(grad_out), _p(idx), _p(out), B, C, int(n), M, _stream()),
               "gather_points_grad")
    return out


def ball_query(new_xyz, xyz, radius, nsample, background=False):
    """background: bq_ball_query_background (same results on about one workgroup per CU: for a query issued ahead of time on
    a second stream, include/bqhip.h)"""
    _req(new_xyz, torch.float32, "new_xyz"); _req(xyz, torch.float32, "xyz"); _same_device(new_xyz, xyz)
    B, M, _ = new_xyz.shape
    N = xyz.shape[1]
    with torch.cuda.device(xyz.device):
        idx = torch.empty(B, M, nsample, dtype=torch.int32, device=xyz.device)
        if N >= BALL_QUERY_GRID_MIN_N[0] and B > 0 and M > 0 and nsample > 0 and radius > 0:
            # large scenes: the same indices through a uniform grid (csrc/ball_query_grid.hip), ~400x fewer distance tests
            nbytes = int(_lib.bq_ball_query_grid_workspace_bytes(B, N))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
            _check(_lib.bq_ball_query_grid(_p(new_xyz), _p(xyz), _p(idx), B, N, M, float(radius), int(nsample), _p(ws), nbytes,
                                           _stream()), "ball_query_grid")
            return idx
        fn = _lib.bq_ball_query_background if background else _lib.bq_ball_query
        _check(fn(_p(new_xyz), _p(xyz), _p(idx), B, N, M, float(radius), int(nsample), _stream()), "ball_query")
    return idx


BALL_QUERY_GRID_MIN_N = [8192]   # scenes from this size on go through the grid (tests / tools set it to compare the two paths)


def ball_query_grid_build_mode(multi):
    """1: the multi-workgroup grid build (default), 0: one workgroup per scene; returns the previous mode (include/bqhip.h)"""
    return int(_lib.bq_ball_query_grid_build_mode(int(multi)))


def group_points(points, idx):
    _req(points, torch.float32, "points"); _req(idx, torch.int32, "idx"); _same_device(points, idx)
    B, C, N = points.shape
    _, M, S = idx.shape
    with torch.cuda.device(points.device):
        out = torch.empty(B, C, M, S, dtype=torch.float32, device=points.device)
        _check(_lib.bq_group_points(_p(points), _p(idx), _p(out), B, C, N, M, S, _stream()), "group_points")
    return out


def group_points_grad(grad_out, idx, n):
    _req(grad_out, torch.float32, "grad_out"); _req(idx, torch.int32, "idx"); _same_device(grad_out, idx)
    B, C, M, S = grad_out.shape
    with torch.cuda.device(grad_out.device):
        out = torch.zeros(B, C, n, dtype=torch.float32, device=grad_out.device)
        _check(_lib.bq_group_points_grad(_p(grad_out), _p(idx), _p(out), B, C, int(n), M, S, _stream()),
               "group_points_grad")
    return out


def three_nn(unknowns, knows):
    _req(unknowns, torch.float32, "unknowns"); _req(knows, torch.float32, "knows"); _same_device(unknowns, knows)
    B, n, _ = unknowns.shape
    m = knows.shape[1]
    with torch.cuda.device(unknowns.device):
        dist2 = torch.empty(B, n, 3, dtype=torch.float32, device=unknowns.device)
        idx = torch.empty(B, n, 3, dtype=torch.int32, device=unknowns.device)
        _check(_lib.bq_three_nn(_p(unknowns), _p(knows), _p(dist2), _p(idx), B, n, m, _stream()), "three_nn")
    return [dist2, idx]


def three_nn_dist(unknowns, knows):
    """three_nn + sqrt in one kernel (IEEE-correct sqrt, unlike the device sqrt torch uses)."""
    _req(unknowns, torch.float32, "unknowns"); _req(knows, torch.float32, "knows"); _same_device(unknowns, knows)
    B, n, _ = unknowns.shape
    m = knows.shape[1]
    with torch.cuda.device(unknowns.device):
        dist = torch.empty(B, n, 3, dtype=torch.float32, device=unknowns.device)
        idx = torch.empty(B, n, 3, dtype=torch.int32, device=unknowns.device)
        _check(_lib.bq_three_nn_dist(_p(unknowns), _p(knows), _p(dist), _p(idx), B, n, m, _stream()), "three_nn_dist")
    return [dist, idx]


def three_interpolate(points, idx, weight):
    _req(points, torch.float32, "points"); _req(idx, torch.int32, "idx"); _req(weight, torch.float32, "weight")
    _same_device(points, idx, weight)
    B, C, m = points.shape
    n = idx.shape[1]
    with torch.cuda.device(points.device):
        out = torch.empty(B, C, n, dtype=torch.float32, device=points.device)
        _check(_lib.bq_three_interpolate(_p(points), _p(idx), _p(weight), _p(out), B, C, m, n, _stream()),
               "three_interpolate")
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    _req(grad_out, torch.float32, "grad_out"); _req(idx, torch.int32, "idx"); _req(weight, torch.float32, "weight")
    _same_device(grad_out, idx, weight)
    B, C, n = grad_out.shape
    with torch.cuda.device(grad_out.device):
        out = torch.zeros(B, C, m, dtype=torch.float32, device=grad_out.device)
        _check(_lib.bq_three_interpolate_grad(_p(grad_out), _p(idx), _p(weight), _p(out), B, C, n, int(m), _stream()),
               "three_interpolate_grad")
    return out


# ---- fused forms (include/bqhip.h) ---------------------------------------------------------------
def group_concat(xyz, new_xyz, features, idx, radius, normalize, out_dtype=torch.float32):
    _req(xyz, torch.float32, "xyz"); _req(new_xyz, torch.float32, "new_xyz"); _req(idx, torch.int32, "idx")
    if features is not None:
        _req(features, torch.float32, "features")
    B, N, _ = xyz.shape
    _, M, S = idx.shape
    C = features.shape[1] if features is not None else 0
    with torch.cuda.device(xyz.device):
        out = torch.empty(B, C + 3, M, S, dtype=out_dtype, device=xyz.device)
        fn = _lib.bq_group_concat_bf16 if out_dtype == torch.bfloat16 else _lib.bq_group_concat
        _check(fn(_p(xyz), _p(new_xyz), _p(features), _p(idx), _p(out), B, C, N, M, S,
                  float(radius), int(bool(normalize)), _stream()), "group_concat")
    return out


def group_concat_grad(grad_out, idx, n, radius, normalize, need_features, need_xyz, need_new_xyz):
    _req(grad_out, grad_out.dtype if grad_out.dtype == torch.bfloat16 else torch.float32, "grad_out")
    _req(idx, torch.int32, "idx")
    B, CT, M, S = grad_out.shape
    C = CT - 3
    dev = grad_out.device
    with torch.cuda.device(dev):
        gf = torch.zeros(B, C, n, dtype=torch.float32, device=dev) if (need_features and C > 0) else None
        gx = torch.zeros(B, n, 3, dtype=torch.float32, device=dev) if need_xyz else None
        gn = torch.zeros(B, M, 3, dtype=torch.float32, device=dev) if need_new_xyz else None
        fn = _lib.bq_group_concat_grad_bf16 if grad_out.dtype == torch.bfloat16 else _lib.bq_group_concat_grad
        _check(fn(_p(grad_out), _p(idx), _p(gf), _p(gx), _p(gn), B, C, int(n), M, S,
                  float(radius), int(bool(normalize)), _stream()), "group_concat_grad")
    return gf, gx, gn


def group_concat_pm(xyz, new_xyz, feats_pm, idx, radius, normalize, out_dtype, pad_to=1):
    """Point-major grouping: feats_pm (B,N,C) f32 view with contiguous rows (any batch / row stride) or None ->
    (B, M, S, 3+C) in out_dtype (f32 / bf16).  pad_to > 1: the rows are allocated with a stride of 3+C rounded up to a
    multiple of pad_to (padding zeroed) and the (B, M, S, 3+C) result is a view of them."""
    _req(xyz, torch.float32, "xyz"); _req(new_xyz, torch.float32, "new_xyz"); _req(idx, torch.int32, "idx")
    B, N, _ = xyz.shape
    _, M, S = idx.shape
    C = 0
    fbs = frs = 0
    if feats_pm is not None:
        if not feats_pm.is_cuda or feats_pm.dtype != torch.float32 or feats_pm.stride(2) != 1:
            raise RuntimeError("feats_pm must be a CUDA float tensor (B,N,C) with contiguous rows")
        C, fbs, frs = feats_pm.shape[2], feats_pm.stride(0), feats_pm.stride(1)
    ld = (C + 3 + pad_to - 1) // pad_to * pad_to
    with torch.cuda.device(xyz.device):
        out = torch.empty(B, M, S, ld, dtype=out_dtype, device=xyz.device)
        _check(_lib.bq_group_concat_pm(_p(xyz), _p(new_xyz), _p(feats_pm), fbs, frs, _p(idx), _p(out),
                                       int(out_dtype == torch.bfloat16), B, C, N, M, S, float(radius),
                                       int(bool(normalize)), ld, _stream()), "group_concat_pm")
    return out[..., :C + 3] if ld != C + 3 else out


def group_concat_pm_grad(grad_out, idx, n, radius, normalize, need_features, need_xyz, need_new_xyz):
    """grad_out (B, M, S, 3+C): contiguous, or a view of rows with a larger uniform stride (the padded rows the
    SharedMLP's input gradient is written in)"""
    B, M, S, CT = grad_out.shape
    C = CT - 3
    dev = grad_out.device
    ld = grad_out.stride(2)
    if grad_out.stride(3) != 1 or grad_out.stride(1) != S * ld or grad_out.stride(0) != M * S * ld or ld < CT:
        grad_out = grad_out.contiguous()
        ld = CT
    with torch.cuda.device(dev):
        gf = torch.zeros(B, n, C, dtype=torch.float32, device=dev) if (need_features and C > 0) else None
        gx = torch.zeros(B, n, 3, dtype=torch.float32, device=dev) if need_xyz else None
        gn = torch.zeros(B, M, 3, dtype=torch.float32, device=dev) if need_new_xyz else None
        _check(_lib.bq_group_concat_pm_grad(_p(grad_out), int(grad_out.dtype == torch.bfloat16), _p(idx), _p(gf),
                                            _p(gx), _p(gn), B, C, int(n), M, S, float(radius),
                                            int(bool(normalize)), ld, _stream()), "group_concat_pm_grad")
    return gf, gx, gn


# ---- fused attention (csrc/attn.hip) ---------------------------------------------------------------
def _bhd_strides(t):
    """(B, L, H, 64) view with a contiguous last dim -> element strides (batch, token, head)."""
    if t.dtype != torch.bfloat16 or t.stride(3) != 1 or t.shape[3] != 64:
        raise RuntimeError("attention operands must be bf16 (B, L, H, 64) views with a contiguous head dim")
    return t.stride(0), t.stride(1), t.stride(2)


LOG2E = 1.4426950408889634


def _pad64(n):
    return (n + 63) // 64 * 64


def key_mask_log2(mask, B, Lk):
    """additive key mask broadcastable to (B,1,1,Lk) -> f32 (B, Lkp), multiplied by log2(e), zero in the padding"""
    if mask is None:
        return None
    m = torch.zeros(B, _pad64(Lk), dtype=torch.float32, device=mask.device)
    m[:, :Lk] = mask.reshape(-1, Lk).expand(B, Lk).float() * LOG2E
    return m


def attn_fwd(q, k, v, scale, mask_log2=None, p_drop=0.0, seed=0, seed_tensor=None, causal=False, out=None):
    """softmax(q k^T * scale + mask) v without materialising the scores.  q: bf16 (B, Lq, H, 64) view, k / v:
    (B, Lk, H, 64) views with equal strides; mask_log2 from key_mask_log2.  Returns out (B, Lq, H, 64) bf16 contiguous
    and lse (B, H, Lq) f32 (log2 domain).  No transposed copies: the kernels transpose out of LDS."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda:
            raise RuntimeError("%s: CPU not supported" % n)
    if k.stride() != v.stride():
        raise RuntimeError("attn_fwd: k and v must have equal strides")
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    Lkp = _pad64(Lk)
    with torch.cuda.device(q.device):
        if out is None:
            out = torch.empty(B, Lq, H, D, dtype=torch.bfloat16, device=q.device)
        elif tuple(out.shape) != (B, Lq, H, D) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise RuntimeError("attn_fwd: out must be a contiguous bf16 (B, Lq, H, 64) tensor")
        lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
        qs, ks, os_ = _bhd_strides(q), _bhd_strides(k), _bhd_strides(out)
        _check(_lib.bq_attn_fwd(_p(q), _p(k), _p(v), _p(out), _p(lse), _p(mask_log2), B, H, Lq, Lk, Lkp, *qs, *ks,
                                *os_, float(scale), float(p_drop), int(seed) & 0xFFFFFFFF, _p(seed_tensor),
                                int(bool(causal)), _stream()), "attn_fwd")
    return out, lse


def attn_probs(q, k, lse, scale, mask_log2=None, p_drop=0.0, seed=0, seed_tensor=None, causal=False):
    """the softmax probabilities of the attn_fwd call that produced `lse`: f32 (B, H, Lq, Lk).  p_drop = 0 (default): the
    map BEFORE dropout, which is what the reference returns (med.py:202,223); with the forward's p_drop / seed: the dropped
    map the context was computed from"""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    with torch.cuda.device(q.device):
        P = torch.empty(B, H, Lq, Lk, dtype=torch.float32, device=q.device)
        qs, ks = _bhd_strides(q), _bhd_strides(k)
        _check(_lib.bq_attn_probs(_p(q), _p(k), _p(lse), _p(mask_log2), _p(P), B, H, Lq, Lk, _pad64(Lk), *qs, *ks,
                                  float(scale), float(p_drop), int(seed) & 0xFFFFFFFF, _p(seed_tensor), int(bool(causal)),
                                  _stream()), "attn_probs")
    return P


def attn_set_persistent(mask):
    """which passes of the unmasked attention use the resident-grid kernels (bit 0 forward, 1 dQ, 2 dK/dV); returns the
    previous mask (include/bqhip_fusion.h: bq_attn_set_persistent)"""
    return int(_lib.bq_attn_set_persistent(int(mask)))


def attn_bwd(q, k, v, out, lse, grad_out, scale, dq, dk, dv, mask_log2=None, p_drop=0.0, seed=0, seed_tensor=None,
             causal=False):
    """Backward of attn_fwd (same mask / dropout arguments).  dq, dk, dv: preallocated bf16 views (dq strided like
    q, dk/dv like k; k and v with equal strides)."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    Lkp = _pad64(Lk)
    if k.stride() != v.stride() or dq.stride() != q.stride() or dk.stride() != k.stride() or dv.stride() != k.stride():
        raise RuntimeError("attn_bwd: stride contract violated")
    with torch.cuda.device(q.device):
        if grad_out.stride(3) != 1 or grad_out.stride(1) % 8 or grad_out.stride(2) % 8:
            grad_out = grad_out.contiguous()
        if not out.is_contiguous():
            raise RuntimeError("attn_bwd: the forward output must be contiguous")
        delta = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)  # filled by the dQ kernel
        qs, ks, gs = _bhd_strides(q), _bhd_strides(k), _bhd_strides(grad_out)
        _check(_lib.bq_attn_bwd(_p(q), _p(k), _p(v), _p(grad_out), _p(lse), _p(out), _p(delta), _p(mask_log2), _p(dq),
                                _p(dk), _p(dv), B, H, Lq, Lk, Lkp, *qs, *ks, *gs, float(scale), float(p_drop),
                                int(seed) & 0xFFFFFFFF, _p(seed_tensor), int(bool(causal)), _stream()), "attn_bwd")


# ---- single-query decode attention over a static cache (csrc/attn_decode.hip) ------------------------------------------------
DECODE_CHUNK = 32        # keys per online-softmax step of attn_decode_kernel (DEC_CHUNK)
DECODE_CALLS = [0, 0]    # launches of attn_decode_self / attn_decode_cross so far (tests assert the route taken)


def _decode_operand(t, shape, name):
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported" % name)
    if t.dtype != torch.bfloat16 or t.dim() != len(shape) or any(w is not None and int(s) != w for s, w in zip(t.shape, shape)):
        raise RuntimeError("%s must be a bf16 tensor of shape %s" % (name, "x".join("*" if w is None else str(w) for w in shape)))
    if t.stride(-1) != 1 or any(st % 8 for st in t.stride()[:-1]) or t.data_ptr() % 16:
        raise RuntimeError("%s must have a contiguous head dim, strides in multiples of 8 and 16-byte alignment" % name)


def _decode_out(out, S, H, like):
    if out is None:
        return torch.empty(S, 1, H, 64, dtype=torch.bfloat16, device=like.device)
    if tuple(out.shape) != (S, 1, H, 64) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != like.device:
        raise RuntimeError("attn_decode: out must be a contiguous bf16 (S, 1, H, 64) tensor on the operands' device")
    return out


def attn_decode_self(qkv, cache, anc, scale, t=0, t_tensor=None, out=None):
    """one decode step of self-attention over a static cache.  qkv: bf16 (S, 1, 3, H, 64) packed projection of the step's token;
    cache: bf16 (S, Lmax, 2, H, 64), row [s, t] is WRITTEN with the step's K / V; anc: int32 (Lmax, S) contiguous, position
    j < t of slot s is cache row anc[j][s]; the position t from t_tensor (int32 device tensor: replayable) or the host value.
    Returns out (S, 1, H, 64) bf16."""
    for x, n in ((qkv, "qkv"), (cache, "cache"), (anc, "anc")):
        if not x.is_cuda:
            raise RuntimeError("attn_decode_self: %s: CPU not supported" % n)
    S, H = qkv.shape[0], qkv.shape[3] if qkv.dim() == 5 else -1
    _decode_operand(qkv, (S, 1, 3, None, 64), "attn_decode_self: qkv")
    _decode_operand(cache, (S, None, 2, H, 64), "attn_decode_self: cache")
    Lmax = cache.shape[1]
    if anc.dtype != torch.int32 or tuple(anc.shape) != (Lmax, S) or not anc.is_contiguous():
        raise RuntimeError("attn_decode_self: anc must be a contiguous int32 (Lmax, S) tensor")
    if t_tensor is not None and (not t_tensor.is_cuda or t_tensor.dtype != torch.int32 or t_tensor.numel() != 1):
        raise RuntimeError("attn_decode_self: t_tensor must be a one-element int32 device tensor")
    if t_tensor is None and not 0 <= int(t) < Lmax:
        raise RuntimeError("attn_decode_self: position %d outside the cache (Lmax %d)" % (t, Lmax))
    _same_device(qkv, cache, anc, *([t_tensor] if t_tensor is not None else []))
    with torch.cuda.device(qkv.device):
        out = _decode_out(out, S, H, qkv)
        DECODE_CALLS[0] += 1
        _check(_lib.bq_attn_decode_self(_p(qkv), _p(cache), _p(anc), _p(out), _p(t_tensor), int(t), S, H, Lmax,
                                        qkv.stride(0), qkv.stride(2), qkv.stride(3), cache.stride(0), cache.stride(1),
                                        cache.stride(2), cache.stride(3), out.stride(0), out.stride(2), float(scale),
                                        _stream()), "attn_decode_self")
    return out


def attn_decode_cross(q, kv, scale, mask_log2=None, out=None):
    """one decode step of cross-attention: q bf16 (S, 1, H, 64) view, kv bf16 (S, Lk, 2, H, 64) by strides (a HoistedKV block),
    mask_log2 from key_mask_log2 ((S, Lkp) f32) or None.  The keys belong to the slot.  Returns out (S, 1, H, 64) bf16."""
    for x, n in ((q, "q"), (kv, "kv")) + (((mask_log2, "mask_log2"),) if mask_log2 is not None else ()):
        if not x.is_cuda:
            raise RuntimeError("attn_decode_cross: %s: CPU not supported" % n)
    S, H = q.shape[0], q.shape[2] if q.dim() == 4 else -1
    _decode_operand(q, (S, 1, None, 64), "attn_decode_cross: q")
    _decode_operand(kv, (S, None, 2, H, 64), "attn_decode_cross: kv")
    Lk, Lkp = kv.shape[1], 0
    if mask_log2 is not None:
        if mask_log2.dtype != torch.float32 or mask_log2.dim() != 2 or mask_log2.shape[0] != S or mask_log2.shape[1] < Lk \
                or not mask_log2.is_contiguous():
            raise RuntimeError("attn_decode_cross: mask_log2 must be a contiguous f32 (S, Lkp >= Lk) tensor")
        Lkp = mask_log2.shape[1]
    _same_device(q, kv, *([mask_log2] if mask_log2 is not None else []))
    if S > 0 and Lk == 0:
        raise RuntimeError("attn_decode_cross: no keys")
    with torch.cuda.device(q.device):
        out = _decode_out(out, S, H, q)
        k, v = kv[:, :, 0], kv[:, :, 1]
        DECODE_CALLS[1] += 1
        _check(_lib.bq_attn_decode_cross(_p(q), _p(k), _p(v), _p(out), _p(mask_log2), S, H, Lk, Lkp, q.stride(0), q.stride(2),
                                         kv.stride(0), kv.stride(1), kv.stride(3), out.stride(0), out.stride(2), float(scale),
                                         _stream()), "attn_decode_cross")
    return out


# ---- one beam-search step on the device (csrc/beam.hip, include/bqhip_beam.h) --------------------------------------------------
BEAM_MAX_NB = _cabi.ADDITIVE_DEFINES["BQ_BEAM_MAX_NB"]      # beams per sample the kernels are built for
BEAM_MAX_LEN = _cabi.ADDITIVE_DEFINES["BQ_BEAM_MAX_LEN"]    # tokens per hypothesis, and rows of the ancestry table
BEAM_CALLS = [0]         # calls of beam_step so far (three launches each; tests assert the route taken)
# bq_beam_state's pointer fields: name -> (dtype, shape as a function of the extents); `logits` is checked apart
_BEAM_FIELDS = {
    "pos": (torch.int32, lambda e: (1,)), "lenpow": (torch.float64, lambda e: (e["max_length"] + 1,)),
    "beam_score": (torch.float32, lambda e: (e["S"],)), "tokens": (torch.int32, lambda e: (e["S"], e["max_length"])),
    "anc": (torch.int32, lambda e: (e["Lmax"], e["S"])), "ids": (torch.int64, lambda e: (e["S"], 1)),
    "done": (torch.int32, lambda e: (e["B"],)), "not_done": (torch.int32, lambda e: (BEAM_MAX_LEN + 2,)),
    "src": (torch.int32, lambda e: (e["S"],)), "cand": (torch.int64, lambda e: (e["S"], 2 * e["nb"])),
    "top_score": (torch.float32, lambda e: (e["B"], 2 * e["nb"])), "top_index": (torch.int32, lambda e: (e["B"], 2 * e["nb"])),
    "heap_len": (torch.int32, lambda e: (e["B"],)), "heap_adds": (torch.int32, lambda e: (e["B"],)),
    "heap_seq": (torch.int32, lambda e: (e["B"], e["nb"])), "heap_hyplen": (torch.int32, lambda e: (e["B"], e["nb"])),
    "heap_sum": (torch.float32, lambda e: (e["B"], e["nb"])), "heap_score": (torch.float64, lambda e: (e["B"], e["nb"])),
    "heap_worst": (torch.float64, lambda e: (e["B"],)), "heap_tokens": (torch.int32, lambda e: (e["B"], e["nb"], e["max_length"])),
}


def beam_state_desc(logits, B, nb, max_length, eos, pad, min_length, early_stopping, **tensors):
    """the bq_beam_state of one decode: logits f32 / bf16 (S, V) with contiguous rows, the extents, and one tensor per pointer
    field of the struct (include/bqhip_beam.h), each checked against the dtype and shape the kernels index it by.  The caller
    keeps the tensors alive as long as it uses the descriptor."""
    if not logits.is_cuda:
        raise RuntimeError("beam_step: logits: CPU not supported")
    S = B * nb
    if logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() != 2 or logits.shape[0] != S or logits.stride(1) != 1 \
            or (S > 1 and logits.stride(0) < logits.shape[1]):
        raise RuntimeError("beam_step: logits must be a float32 or bfloat16 (B * nb, V) tensor with contiguous rows")
    V = logits.shape[1]
    if "anc" not in tensors or tensors["anc"].dim() != 2:
        raise RuntimeError("beam_step: anc must be an int32 (Lmax, S) tensor")
    e = dict(B=B, nb=nb, S=S, V=V, max_length=int(max_length), Lmax=tensors["anc"].shape[0])
    if not (1 <= nb <= BEAM_MAX_NB and V >= 2 * nb and nb * V < 2 ** 31 and 1 <= e["max_length"] <= BEAM_MAX_LEN
            and 1 <= e["Lmax"] <= BEAM_MAX_LEN and 0 <= eos < V and 0 <= pad < V and B >= 1):
        raise RuntimeError("beam_step: bad extents (B %d, nb %d, V %d, max_length %d, Lmax %d, eos %d, pad %d)"
                           % (B, nb, V, e["max_length"], e["Lmax"], eos, pad))
    if set(tensors) != set(_BEAM_FIELDS):
        raise RuntimeError("beam_step: the state needs exactly the tensors %s" % sorted(_BEAM_FIELDS))
    for name, (dtype, shape) in _BEAM_FIELDS.items():
        t = tensors[name]
        if not t.is_cuda:
            raise RuntimeError("beam_step: %s: CPU not supported" % name)
        if t.dtype != dtype or tuple(t.shape) != shape(e) or not t.is_contiguous():
            raise RuntimeError("beam_step: %s must be a contiguous %s tensor of shape %s" % (name, dtype, shape(e)))
    _same_device(logits, *tensors.values())
    desc = _cabi.ADDITIVE_STRUCTS["bq_beam_state"](
        B=B, nb=nb, V=V, max_length=e["max_length"], Lmax=e["Lmax"], eos=int(eos), pad=int(pad), min_length=int(min_length),
        early_stopping=int(bool(early_stopping)), logits_bf16=int(logits.dtype == torch.bfloat16),
        ld_logits=logits.stride(0) if S > 1 else V, logits=_p(logits), **{n: _p(t) for n, t in tensors.items()})
    return desc


def beam_step(desc, device):
    """one step of bqx_beam_step on the current stream of `device`: allocates nothing, synchronises nothing (capturable)"""
    with torch.cuda.device(device):
        BEAM_CALLS[0] += 1
        _check(_lib.bqx_beam_step(ctypes.byref(desc), _stream()), "beam_step")


# ---- the LSTM recurrence of the question branch (csrc/lstm.hip) ---------------------------------------------------------------
LSTM_HIDDEN = (128, 256)   # hidden sizes lstm_fwd_kernel / lstm_bwd_kernel are built for
LSTM_CALLS = [0, 0]        # launches of lstm_fwd / lstm_bwd so far (tests assert the route taken)


def _lstm_operand(t, shape, name, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported" % name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s must be a %s tensor of shape %s, got %s %s" % (name, str(dtype).replace("torch.", ""),
                                                                            tuple(shape), t.dtype, tuple(t.shape)))
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)


def _lstm_hidden(H, what):
    if H not in LSTM_HIDDEN:
        raise RuntimeError("%s: hidden size %d is not built (supported: %s)" % (what, H, ", ".join(map(str, LSTM_HIDDEN))))


def lstm_fwd(gx, wt, lens, t_out, reverse=False, save=False):
    """the recurrence of one LSTM layer and direction.  gx: f32 (B, T, 4H) = x W_ih^T + b_ih + b_hh (gate order i f g o); wt: f32
    (H, 4H) = W_hh^T; lens: int32 (B) on the device, clamped to [0, t_out] by the kernel; t_out <= T.  Returns y (B, t_out, H)
    with rows t >= lens[b] zero, h_last (B, H), and with `save` the post-activation gates (B, t_out, 4H) and cell states
    (B, t_out, H) that lstm_bwd reads (else None, None).  Every check is made before the launch."""
    for x, n in ((gx, "gx"), (wt, "wt"), (lens, "lens")):
        if not x.is_cuda:
            raise RuntimeError("lstm_fwd: %s: CPU not supported" % n)
    if gx.dim() != 3 or gx.shape[2] % 4:
        raise RuntimeError("lstm_fwd: gx must be (B, T, 4H)")
    B, T, H = gx.shape[0], gx.shape[1], gx.shape[2] // 4
    _lstm_hidden(H, "lstm_fwd")
    _lstm_operand(gx, (B, T, 4 * H), "lstm_fwd: gx")
    _lstm_operand(wt, (H, 4 * H), "lstm_fwd: wt")
    _lstm_operand(lens, (B,), "lstm_fwd: lens", torch.int32)
    t_out = int(t_out)
    if not 0 <= t_out <= T:
        raise RuntimeError("lstm_fwd: t_out %d outside [0, T = %d]" % (t_out, T))
    _same_device(gx, wt, lens)
    with torch.cuda.device(gx.device):
        y = torch.empty(B, t_out, H, dtype=torch.float32, device=gx.device)
        h_last = torch.empty(B, H, dtype=torch.float32, device=gx.device)
        gates = torch.empty(B, t_out, 4 * H, dtype=torch.float32, device=gx.device) if save else None
        cells = torch.empty(B, t_out, H, dtype=torch.float32, device=gx.device) if save else None
        LSTM_CALLS[0] += 1
        _check(_lib.bq_lstm_fwd(_p(gx), _p(wt), _p(lens), _p(y), _p(h_last), _p(gates), _p(cells), B, T, t_out, H,
                                int(bool(reverse)), _stream()), "lstm_fwd")
    return y, h_last, gates, cells


def lstm_bwd(dy, dh_last, gates, cells, w_hh, lens, reverse=False):
    """gradient of the pre-activation gates.  dy: f32 (B, t_out, H) or None; dh_last: f32 (B, H) or None; gates / cells as
    lstm_fwd saved them; w_hh: f32 (4H, H) as nn.LSTM holds it; lens as in lstm_fwd.  Returns dgx (B, t_out, 4H) with rows
    t >= lens[b] zero."""
    for x, n in ((dy, "dy"), (dh_last, "dh_last"), (gates, "gates"), (cells, "cells"), (w_hh, "w_hh"), (lens, "lens")):
        if x is not None and not x.is_cuda:
            raise RuntimeError("lstm_bwd: %s: CPU not supported" % n)
    if cells.dim() != 3:
        raise RuntimeError("lstm_bwd: cells must be (B, t_out, H)")
    B, t_out, H = cells.shape
    _lstm_hidden(H, "lstm_bwd")
    _lstm_operand(cells, (B, t_out, H), "lstm_bwd: cells")
    _lstm_operand(gates, (B, t_out, 4 * H), "lstm_bwd: gates")
    _lstm_operand(w_hh, (4 * H, H), "lstm_bwd: w_hh")
    _lstm_operand(lens, (B,), "lstm_bwd: lens", torch.int32)
    if dy is not None:
        _lstm_operand(dy, (B, t_out, H), "lstm_bwd: dy")
    if dh_last is not None:
        _lstm_operand(dh_last, (B, H), "lstm_bwd: dh_last")
    _same_device(cells, gates, w_hh, lens, *[x for x in (dy, dh_last) if x is not None])
    with torch.cuda.device(cells.device):
        dgx = torch.empty(B, t_out, 4 * H, dtype=torch.float32, device=cells.device)
        LSTM_CALLS[1] += 1
        _check(_lib.bq_lstm_bwd(_p(dy), _p(dh_last), _p(gates), _p(cells), _p(w_hh), _p(lens), _p(dgx), B, t_out, H,
                                int(bool(reverse)), _stream()), "lstm_bwd")
    return dgx


# ---- the row operators of the MCAN blocks: residual LayerNorm and AttFlat pooling (csrc/mcan.hip, include/bqhip_mcan.h) -----------
MCAN_MAX_H = _cabi.ADDITIVE_DEFINES["BQ_MCAN_MAX_H"]
MCAN_MAX_N = _cabi.ADDITIVE_DEFINES["BQ_MCAN_MAX_N"]
MCAN_MAX_G = _cabi.ADDITIVE_DEFINES["BQ_MCAN_MAX_G"]
MCAN_CALLS = [0, 0, 0, 0]  # launches of mcan_ln_fwd / mcan_ln_bwd / attflat_pool_fwd / attflat_pool_bwd so far


def mcan_hidden_ok(H):
    """the row lengths the kernels of csrc/mcan.hip are built for: multiples of 64 from 64 to MCAN_MAX_H"""
    return 64 <= H <= MCAN_MAX_H and H % 64 == 0


def _mcan_operands(what, items):
    """items: (tensor or None, shape, name, dtype); a CPU tensor raises first, as everywhere in this module"""
    for t, _, n, _ in items:
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s: %s: CPU not supported" % (what, n))
    for t, shape, n, dtype in items:
        if t is not None:
            _lstm_operand(t, shape, "%s: %s" % (what, n), dtype)
    _same_device(*[t for t, _, _, _ in items if t is not None])


def _mcan_hidden(H, what):
    if not mcan_hidden_ok(H):
        raise RuntimeError("%s: row length %d is not built (a multiple of 64 in [64, %d])" % (what, H, MCAN_MAX_H))


def mcan_ln_fwd(x, s, a2, b2, eps):
    """MCAN's LayerNorm of z = x + s (s None: z = x): y = a2 (z - mean) / (sigma + eps) + b2 with the unbiased deviation.  x, s:
    f32 (M, H); a2, b2: f32 (H).  Returns y (M, H), mean (M), sigma (M) -- what mcan_ln_bwd reads."""
    if not x.is_cuda:
        raise RuntimeError("mcan_ln_fwd: x: CPU not supported")
    if x.dim() != 2:
        raise RuntimeError("mcan_ln_fwd: x must be (M, H)")
    M, H = x.shape
    _mcan_operands("mcan_ln_fwd", ((x, (M, H), "x", torch.float32), (s, (M, H), "s", torch.float32),
                                   (a2, (H,), "a2", torch.float32), (b2, (H,), "b2", torch.float32)))
    _mcan_hidden(H, "mcan_ln_fwd")
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        sigma = torch.empty(M, dtype=torch.float32, device=x.device)
        MCAN_CALLS[0] += 1
        _check(_lib.bqm_mcan_ln_fwd(_p(x), _p(s), _p(a2), _p(b2), _p(y), _p(mean), _p(sigma), M, H, float(eps), _stream()),
               "mcan_ln_fwd")
    return y, mean, sigma


def mcan_ln_bwd(dy, x, s, a2, mean, sigma, eps):
    """gradients of mcan_ln_fwd.  Returns dz (M, H) -- the gradient of x and of s alike -- and dab (2, H) = [da2, db2], stored
    (not accumulated) by a fixed-order fold over a slab allocated here."""
    if not dy.is_cuda:
        raise RuntimeError("mcan_ln_bwd: dy: CPU not supported")
    if dy.dim() != 2:
        raise RuntimeError("mcan_ln_bwd: dy must be (M, H)")
    M, H = dy.shape
    _mcan_operands("mcan_ln_bwd", ((dy, (M, H), "dy", torch.float32), (x, (M, H), "x", torch.float32),
                                   (s, (M, H), "s", torch.float32), (a2, (H,), "a2", torch.float32),
                                   (mean, (M,), "mean", torch.float32), (sigma, (M,), "sigma", torch.float32)))
    _mcan_hidden(H, "mcan_ln_bwd")
    with torch.cuda.device(dy.device):
        dz = torch.empty_like(dy)
        if M == 0:
            return dz, torch.zeros(2, H, dtype=torch.float32, device=dy.device)
        dab = torch.empty(2, H, dtype=torch.float32, device=dy.device)
        slab = torch.empty(_lib.bqm_mcan_ln_bwd_slab_floats(M, H), dtype=torch.float32, device=dy.device)
        MCAN_CALLS[1] += 1
        _check(_lib.bqm_mcan_ln_bwd(_p(dy), _p(x), _p(s), _p(a2), _p(mean), _p(sigma), _p(dz), _p(dab), _p(slab), M, H,
                                    float(eps), _stream()), "mcan_ln_bwd")
    return dz, dab


def _pool_extents(x, what):
    if x.dim() != 3:
        raise RuntimeError("%s: x must be (B, N, H)" % what)
    return x.shape


def _pool_limits(N, G, H, what):
    _mcan_hidden(H, what)
    if not (1 <= N <= MCAN_MAX_N and 1 <= G <= MCAN_MAX_G):
        raise RuntimeError("%s: N %d, G %d are not built (1 <= N <= %d, 1 <= G <= %d)" % (what, N, G, MCAN_MAX_N, MCAN_MAX_G))


def attflat_pool_fwd(x, logits, hide=None):
    """AttFlat's tail: p = softmax over the keys of (hide ? -1e9 : logits), out[b, g H + h] = sum_n p[b, n, g] x[b, n, h].
    x: f32 (B, N, H); logits: f32 (B, N, G); hide: uint8 (B, N), non-zero = hidden, or None.  Returns out (B, G H), p (B, N, G)."""
    if not x.is_cuda:
        raise RuntimeError("attflat_pool_fwd: x: CPU not supported")
    B, N, H = _pool_extents(x, "attflat_pool_fwd")
    if logits.dim() != 3:
        raise RuntimeError("attflat_pool_fwd: logits must be (B, N, G)")
    G = logits.shape[2]
    _mcan_operands("attflat_pool_fwd", ((x, (B, N, H), "x", torch.float32), (logits, (B, N, G), "logits", torch.float32),
                                        (hide, (B, N), "hide", torch.uint8)))
    _pool_limits(N, G, H, "attflat_pool_fwd")
    with torch.cuda.device(x.device):
        out = torch.empty(B, G * H, dtype=torch.float32, device=x.device)
        p = torch.empty(B, N, G, dtype=torch.float32, device=x.device)
        MCAN_CALLS[2] += 1
        _check(_lib.bqm_attflat_pool_fwd(_p(x), _p(logits), _p(hide), _p(out), _p(p), B, N, G, H, _stream()), "attflat_pool_fwd")
    return out, p


def attflat_pool_bwd(dout, x, p, hide=None):
    """gradients of attflat_pool_fwd: dx (B, N, H) and dlogits (B, N, G), exactly 0 where hide is set"""
    if not dout.is_cuda:
        raise RuntimeError("attflat_pool_bwd: dout: CPU not supported")
    B, N, H = _pool_extents(x, "attflat_pool_bwd")
    if p.dim() != 3:
        raise RuntimeError("attflat_pool_bwd: p must be (B, N, G)")
    G = p.shape[2]
    _mcan_operands("attflat_pool_bwd", ((dout, (B, G * H), "dout", torch.float32), (x, (B, N, H), "x", torch.float32),
                                        (p, (B, N, G), "p", torch.float32), (hide, (B, N), "hide", torch.uint8)))
    _pool_limits(N, G, H, "attflat_pool_bwd")
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dlogits = torch.empty_like(p)
        MCAN_CALLS[3] += 1
        _check(_lib.bqm_attflat_pool_bwd(_p(dout), _p(x), _p(p), _p(hide), _p(dx), _p(dlogits), B, N, G, H, _stream()),
               "attflat_pool_bwd")
    return dx, dlogits


# ---- the attention core of the MCAN blocks' MHAtt (csrc/mhatt.hip, include/bqhip_mhatt.h) -----------------------------------------
MHATT_MAX_N = _cabi.ADDITIVE_DEFINES["BQ_MHATT_MAX_N"]
MHATT_HEAD = (32, 64)
MHATT_CALLS = [0, 0]  # launches of mhatt_fwd / mhatt_bwd so far


def mhatt_ok(H, heads, Nq, Nk):
    """the sizes the kernels of csrc/mhatt.hip are built for: H = heads d with d 32 or 64, 1 <= Nq, Nk <= MHATT_MAX_N"""
    return heads >= 1 and H % heads == 0 and H // heads in MHATT_HEAD and 1 <= Nq <= MHATT_MAX_N and 1 <= Nk <= MHATT_MAX_N


def _mhatt_extents(q, k, heads, what):
    if q.dim() != 3 or k.dim() != 3:
        raise RuntimeError("%s: q must be (B, Nq, H) and k (B, Nk, H)" % what)
    B, Nq, H = q.shape
    Nk, heads = k.shape[1], int(heads)
    if not mhatt_ok(H, heads, Nq, Nk):
        raise RuntimeError("%s: H %d, heads %d, Nq %d, Nk %d are not built (H / heads in %s, 1 <= Nq, Nk <= %d)" % (
            what, H, heads, Nq, Nk, MHATT_HEAD, MHATT_MAX_N))
    if B * heads > 65535:
        raise RuntimeError("%s: B heads = %d is not built (at most 65535)" % (what, B * heads))
    return B, heads, Nq, Nk, H


def mhatt_fwd(q, k, v, hide, keep, heads):
    """MHAtt's core on the linears' outputs as they stand.  q: f32 (B, Nq, H); k, v: f32 (B, Nk, H), head h in columns
    [h d, (h + 1) d); hide: uint8 (B, Nk), non-zero = hidden key, or None; keep: f32 (B, heads, Nq, Nk), the dropout multiplier,
    or None.  Returns out (B, Nq, H) = softmax(hide ? -1e9 : q k^T / sqrt d) keep v per head and p (B, heads, Nq, Nk), the
    probabilities before keep -- what mhatt_bwd reads."""
    if not q.is_cuda:
        raise RuntimeError("mhatt_fwd: q: CPU not supported")
    B, heads, Nq, Nk, H = _mhatt_extents(q, k, heads, "mhatt_fwd")
    _mcan_operands("mhatt_fwd", ((q, (B, Nq, H), "q", torch.float32), (k, (B, Nk, H), "k", torch.float32),
                                 (v, (B, Nk, H), "v", torch.float32), (hide, (B, Nk), "hide", torch.uint8),
                                 (keep, (B, heads, Nq, Nk), "keep", torch.float32)))
    with torch.cuda.device(q.device):
        out = torch.empty_like(q)
        p = torch.empty(B, heads, Nq, Nk, dtype=torch.float32, device=q.device)
        MHATT_CALLS[0] += 1
        _check(_lib.bqh_mhatt_fwd(_p(q), _p(k), _p(v), _p(hide), _p(keep), _p(out), _p(p), B, heads, Nq, Nk, H // heads,
                                  _stream()), "mhatt_fwd")
    return out, p


def mhatt_bwd(dout, q, k, v, p, hide, keep, heads):
    """gradients of mhatt_fwd from p as saved: dq (B, Nq, H), dk and dv (B, Nk, H), each element stored once in a fixed order of
    additions; dq and dk pass nothing through a hidden key.  The (B, heads, Nq, Nk) workspace is allocated here."""
    if not dout.is_cuda:
        raise RuntimeError("mhatt_bwd: dout: CPU not supported")
    B, heads, Nq, Nk, H = _mhatt_extents(q, k, heads, "mhatt_bwd")
    _mcan_operands("mhatt_bwd", ((dout, (B, Nq, H), "dout", torch.float32), (q, (B, Nq, H), "q", torch.float32),
                                 (k, (B, Nk, H), "k", torch.float32), (v, (B, Nk, H), "v", torch.float32),
                                 (p, (B, heads, Nq, Nk), "p", torch.float32), (hide, (B, Nk), "hide", torch.uint8),
                                 (keep, (B, heads, Nq, Nk), "keep", torch.float32)))
    d = H // heads
    with torch.cuda.device(dout.device):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty(max(1, _lib.bqh_mhatt_bwd_ws_floats(B, heads, Nq, Nk, d)), dtype=torch.float32, device=dout.device)
        MHATT_CALLS[1] += 1
        _check(_lib.bqh_mhatt_bwd(_p(dout), _p(q), _p(k), _p(v), _p(p), _p(hide), _p(keep), _p(dq), _p(dk), _p(dv), _p(ws), B,
                                  heads, Nq, Nk, d, _stream()), "mhatt_bwd")
    return dq, dk, dv


# ---- training-scene preparation: sample, augment, vote labels (csrc/scene_prep.hip, include/bqhip_scene.h) -----------------------
SCENE_XF = _cabi.ADDITIVE_DEFINES["BQ_SCENE_XF"]             # doubles per sample: flips, Rx, Ry, Rz, t, Rz Ry Rx
SCENE_ENTRY = _cabi.ADDITIVE_DEFINES["BQ_SCENE_ENTRY"]       # unsigneds per (sample, instance id) of the min / max / first table
SCENE_MAX_IDS = _cabi.ADDITIVE_DEFINES["BQ_SCENE_MAX_IDS"]   # instance ids 0 .. SCENE_MAX_IDS - 1
SCENE_CALLS = [0, 0, 0]    # launches of scene_boxes / scene_sample / scene_votes so far (tests count launches per batch)


def _scene_operand(t, shape, dtype, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("scene_prep: %s: CPU not supported (a device tensor is needed)" % name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise RuntimeError("scene_prep: %s must be a %s tensor of shape %s, got %s %s"
                           % (name, str(dtype).replace("torch.", ""), tuple(shape), t.dtype, tuple(t.shape)))
    if not t.is_contiguous():
        raise RuntimeError("scene_prep: %s must be a contiguous tensor" % name)


def scene_prep(store, scene, object_id, choices, xf, out, table, augment=True, check=False):
    """one batch of training scenes in three launches.  store: the device tensors of scene_data.SceneStore (rows (sum P, D) f32,
    inst / sem (sum P) i32, row_base (S + 1) i64, boxes (S, G, 8) f64, num_bbox (S) i32, box_class (S, G) i32, mean_size (NC, 3)
    f64, votes_sem (L) u8); scene / object_id (B) i32; choices (B, N) i32; xf (B, SCENE_XF) f64 (None without augment); out: every
    key of scene_data.out_spec, preallocated; table (B, T, SCENE_ENTRY) i32 scratch.  Nothing is allocated and the host does not wait,
    unless check=True: then choices outside [0, P_scene) and scene indices outside [0, S) raise (one device-to-host read); without
    it the kernels clamp them.  Every check is made before the first launch."""
    rows = store.rows
    if not torch.is_tensor(rows) or not rows.is_cuda or rows.dim() != 2:
        raise RuntimeError("scene_prep: rows: CPU not supported (a 2-d device tensor is needed)")
    if not torch.is_tensor(choices) or choices.dim() != 2:
        raise RuntimeError("scene_prep: choices must be (B, N)")
    (Ptot, D), (B, N) = rows.shape, choices.shape
    S, G, NC, L = store.row_base.shape[0] - 1, store.boxes.shape[1], store.mean_size.shape[0], store.votes_sem.shape[0]
    T = table.shape[1] if torch.is_tensor(table) and table.dim() == 3 else 0
    for t, shape, dtype, name in ((rows, (Ptot, D), torch.float32, "rows"), (store.inst, (Ptot,), torch.int32, "inst"),
                                  (store.sem, (Ptot,), torch.int32, "sem"), (store.row_base, (S + 1,), torch.int64, "row_base"),
                                  (store.boxes, (S, G, 8), torch.float64, "boxes"), (store.num_bbox, (S,), torch.int32, "num_bbox"),
                                  (store.box_class, (S, G), torch.int32, "box_class"),
                                  (store.mean_size, (NC, 3), torch.float64, "mean_size"),
                                  (store.votes_sem, (L,), torch.uint8, "votes_sem"), (scene, (B,), torch.int32, "scene"),
                                  (object_id, (B,), torch.int32, "object_id"), (choices, (B, N), torch.int32, "choices"),
                                  (table, (B, T, SCENE_ENTRY), torch.int32, "table")):
        _scene_operand(t, shape, dtype, name)
    if augment:
        _scene_operand(xf, (B, SCENE_XF), torch.float64, "xf")
    from .scene_data import out_spec   # (imports nothing of this module at load time)
    spec = out_spec(B, N, D, G, augment)
    for k, (shape, dtype) in spec.items():
        if k not in out:
            raise RuntimeError("scene_prep: out has no %r" % k)
        _scene_operand(out[k], shape, dtype, "out[%r]" % k)
    _same_device(rows, store.inst, store.sem, store.row_base, store.boxes, store.num_bbox, store.box_class, store.mean_size,
                 store.votes_sem, scene, object_id, choices, table, *([xf] if augment else []), *[out[k] for k in spec])
    if not 1 <= T <= SCENE_MAX_IDS:
        raise RuntimeError("scene_prep: table holds %d entries per sample (1 .. %d)" % (T, SCENE_MAX_IDS))
    with torch.cuda.device(rows.device):
        if check:
            sl = scene.long()
            ok_s = (sl >= 0) & (sl < S)
            sl = sl.clamp(0, S - 1)
            P = (store.row_base[sl + 1] - store.row_base[sl])[:, None]
            bad = int((~ok_s).sum()), int(((choices < 0) | (choices >= P)).sum())
            if bad[0] or bad[1]:
                raise RuntimeError("scene_prep: %d scene indices outside [0, %d), %d choices outside [0, P of their scene)"
                                   % (bad[0], S, bad[1]))
        o = lambda k: _p(out[k]) if k in spec else None
        st = _stream()
        SCENE_CALLS[0] += 1
        _check(_lib.bq_scene_boxes(_p(store.boxes), _p(store.num_bbox), _p(store.box_class), _p(store.mean_size), _p(scene),
                                   _p(object_id), _p(xf) if augment else None, o("target_bboxes"), o("center_label"),
                                   o("size_residual_label"), o("heading_residual_label"), o("box_label_mask"),
                                   o("heading_class_label"), o("size_class_label"), o("sem_cls_label"), o("ref_box_label"),
                                   o("num_bbox"), o("ref_obj_mask"), o("ref_center_label"), o("ref_size_class_label"),
                                   o("ref_size_residual_label"), o("flip_x"), o("flip_y"), o("rot_mat"), o("translation"),
                                   _p(table), S, G, NC, B, T, int(bool(augment)), st), "scene_boxes")
        SCENE_CALLS[1] += 1
        _check(_lib.bq_scene_sample(_p(rows), _p(store.inst), _p(store.row_base), _p(scene), _p(choices),
                                    _p(xf) if augment else None, o("point_clouds"), _p(table), S, B, N, D, T,
                                    int(bool(augment)), st), "scene_sample")
        SCENE_CALLS[2] += 1
        _check(_lib.bq_scene_votes(_p(store.inst), _p(store.sem), _p(store.votes_sem), _p(store.row_base), _p(scene), _p(choices),
                                   o("point_clouds"), _p(table), o("vote_label"), o("vote_label_mask"), S, B, N, D, T, L, st),
               "scene_votes")
    return out


# ---- image views: Pillow-exact bicubic resize and normalise (csrc/view_prep.hip, include/bqhip_view.h) ----------------------------
VIEW_COLS = _cabi.ADDITIVE_DEFINES["BQ_VIEW_COLS"]             # long longs per view: first byte, H, W, horizontal / vertical table
VIEW_DESC = _cabi.ADDITIVE_DEFINES["BQ_VIEW_DESC"]             # int32s per table: bounds offset, coefficient offset, ksize, extent
VIEW_LDS_BYTES = _cabi.ADDITIVE_DEFINES["BQ_VIEW_LDS_BYTES"]   # LDS of a workgroup: 4096 for the table + 3 OW bytes per input row
VIEW_CALLS = [0]           # launches of view_prep so far


def _view_operand(t, shape, dtype, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("view_prep: %s: CPU not supported (a device tensor is needed)" % name)
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError("view_prep: %s must be a %s tensor of shape %s, got %s %s"
                           % (name, str(dtype).replace("torch.", ""), shape and tuple(shape), t.dtype, tuple(t.shape)))
    if not t.is_contiguous():
        raise RuntimeError("view_prep: %s must be a contiguous tensor" % name)


def view_prep(pixels, views, tab, desc, index, norm, out, OH, OW, tile_rows, lds_rows, patch=0):
    """one batch of image views in one launch.  pixels (bytes) u8; views (NV, VIEW_COLS) i64; tab (n) i32 and desc (NT, VIEW_DESC)
    i32: the coefficient tables; index (B) i64; norm (3, 256) f32 or bf16, which decides the output type; out: (B, 3, OH, OW), or
    (B, OH OW / patch^2, 3 patch^2) with patch > 0, of norm's dtype.  Nothing is allocated and the host does not wait."""
    if not torch.is_tensor(norm) or norm.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("view_prep: norm must be a float32 or bfloat16 tensor")
    if not torch.is_tensor(index) or index.dim() != 1:
        raise RuntimeError("view_prep: index must be (B,)")
    OH, OW, patch, B = int(OH), int(OW), int(patch), index.shape[0]
    if patch < 0 or (patch and (OH % patch or OW % patch)):
        raise RuntimeError("view_prep: patch = %d does not divide the output %d x %d" % (patch, OH, OW))
    oshape = (B, (OH // patch) * (OW // patch), 3 * patch * patch) if patch else (B, 3, OH, OW)
    for t, shape, dtype, name in ((pixels, None, torch.uint8, "pixels"), (views, None, torch.int64, "views"),
                                  (tab, None, torch.int32, "tab"), (desc, None, torch.int32, "desc"),
                                  (index, (B,), torch.int64, "index"), (norm, (3, 256), norm.dtype, "norm"),
                                  (out, oshape, norm.dtype, "out")):
        _view_operand(t, shape, dtype, name)
    if views.dim() != 2 or views.shape[1] != VIEW_COLS or desc.dim() != 2 or desc.shape[1] != VIEW_DESC or tab.dim() != 1 \
            or pixels.dim() != 1:
        raise RuntimeError("view_prep: pixels (n,), views (NV, %d), tab (n,) and desc (NT, %d) are needed" % (VIEW_COLS, VIEW_DESC))
    _same_device(pixels, views, tab, desc, index, norm, out)
    with torch.cuda.device(pixels.device):
        VIEW_CALLS[0] += 1
        _check(_lib.bq_view_prep(_p(pixels), pixels.shape[0], _p(views), views.shape[0], _p(tab), _p(desc), desc.shape[0],
                                 tab.shape[0], _p(index), B, _p(norm), _p(out), OH, OW, int(tile_rows), int(lds_rows),
                                 int(norm.dtype == torch.bfloat16), patch, _stream()), "view_prep")
    return out


# ---- attention of answer ranking: candidate sequences sharing their question's K / V (csrc/attn_rank.hip) -------------------------
RANK_LMAX = _D["BQ_RANK_LMAX"]       # tokens per sequence attn_rank_self holds in registers
RANK_QBLOCK = _D["BQ_RANK_QBLOCK"]   # queries a wave of attn_rank_cross carries through one loaded K / V chunk
RANK_CALLS = [0, 0]    # launches of attn_rank_self / attn_rank_cross that the library accepted (tests assert the route taken)
# (contract of both wrappers, relied on by tests/test_attn_rank_cpu.py: between the is_cuda checks and the last operand check
# nothing touches the device -- only shape, dtype, stride and data_ptr are read)


def _rank_mask(mask_log2, rows, keys, name, what):
    if mask_log2 is None:
        return 0
    if mask_log2.dtype != torch.float32 or mask_log2.dim() != 2 or mask_log2.shape[0] != rows or mask_log2.shape[1] < keys \
            or not mask_log2.is_contiguous():
        raise RuntimeError("%s: mask_log2 must be a contiguous f32 %s tensor" % (name, what))
    return mask_log2.shape[1]


def _rank_out(out, N, La, H, like, name):
    if out is None:
        return torch.empty(N, La, H, 64, dtype=torch.bfloat16, device=like.device)
    if tuple(out.shape) != (N, La, H, 64) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != like.device:
        raise RuntimeError("%s: out must be a contiguous bf16 (N, La, H, 64) tensor on the operands' device" % name)
    return out


def attn_rank_self(qkv, scale, mask_log2=None, out=None):
    """causal self-attention of N short sequences on their packed projection.  qkv: bf16 (N, La, 3, H, 64) by strides (as
    multi_linear writes it), La <= RANK_LMAX; mask_log2 from key_mask_log2 ((N, Lap >= La) f32, finite) or None: query i sees
    key j iff j <= i, the key mask on top.  Returns out (N, La, H, 64) bf16."""
    for x, n in ((qkv, "qkv"),) + (((mask_log2, "mask_log2"),) if mask_log2 is not None else ()):
        if not x.is_cuda:
            raise RuntimeError("attn_rank_self: %s: CPU not supported" % n)
    N, La, H = (qkv.shape[0], qkv.shape[1], qkv.shape[3]) if qkv.dim() == 5 else (-1, -1, -1)
    _decode_operand(qkv, (N, La, 3, None, 64), "attn_rank_self: qkv")
    if La > RANK_LMAX:
        raise RuntimeError("attn_rank_self: %d tokens per sequence, the kernel holds %d" % (La, RANK_LMAX))
    if N > 0 and La == 0:
        raise RuntimeError("attn_rank_self: no tokens")
    Lap = _rank_mask(mask_log2, N, La, "attn_rank_self", "(N, Lap >= La)")
    _same_device(qkv, *([mask_log2] if mask_log2 is not None else []))
    with torch.cuda.device(qkv.device):
        out = _rank_out(out, N, La, H, qkv, "attn_rank_self")
        _check(_lib.bq_attn_rank_self(_p(qkv), _p(out), _p(mask_log2), N, H, La, Lap, qkv.stride(0), qkv.stride(1),
                                      qkv.stride(2), qkv.stride(3), out.stride(0), out.stride(1), out.stride(2), float(scale),
                                      _stream()), "attn_rank_self")
        RANK_CALLS[0] += 1
    return out


def attn_rank_cross(q, kv, scale, group, mask_log2=None, out=None):
    """cross-attention of N = Bq * group sequences over the keys / values of their question: q bf16 (N, La, H, 64) view, kv bf16
    (Bq, Lk, 2, H, 64) by strides (a HoistedKV block over the UNTILED question states), sequence n reads question n // group;
    mask_log2 from key_mask_log2 ((Bq, Lkp >= Lk) f32) or None.  Returns out (N, La, H, 64) bf16."""
    for x, n in ((q, "q"), (kv, "kv")) + (((mask_log2, "mask_log2"),) if mask_log2 is not None else ()):
        if not x.is_cuda:
            raise RuntimeError("attn_rank_cross: %s: CPU not supported" % n)
    N, La, H = (q.shape[0], q.shape[1], q.shape[2]) if q.dim() == 4 else (-1, -1, -1)
    _decode_operand(q, (N, La, None, 64), "attn_rank_cross: q")
    _decode_operand(kv, (None, None, 2, H, 64), "attn_rank_cross: kv")
    Bq, Lk = kv.shape[0], kv.shape[1]
    group = int(group)
    if group < 1 or Bq * group != N:
        raise RuntimeError("attn_rank_cross: group %d: %d sequences are not %d questions x group" % (group, N, Bq))
    Lkp = _rank_mask(mask_log2, Bq, Lk, "attn_rank_cross", "(Bq, Lkp >= Lk)")
    _same_device(q, kv, *([mask_log2] if mask_log2 is not None else []))
    if N > 0 and (Lk == 0 or La == 0):
        raise RuntimeError("attn_rank_cross: no keys or no queries")
    with torch.cuda.device(q.device):
        out = _rank_out(out, N, La, H, q, "attn_rank_cross")
        k, v = kv[:, :, 0], kv[:, :, 1]
        _check(_lib.bq_attn_rank_cross(_p(q), _p(k), _p(v), _p(out), _p(mask_log2), N, Bq, group, H, La, Lk, Lkp, q.stride(0),
                                       q.stride(1), q.stride(2), kv.stride(0), kv.stride(1), kv.stride(3), out.stride(0),
                                       out.stride(1), out.stride(2), float(scale), _stream()), "attn_rank_cross")
        RANK_CALLS[1] += 1
    return out


_AttnSide = _cabi.STRUCTS["bq_attn_side"]


def attn_pair_ok(qa, ka, qb, kb):
    """both attentions qualify for the narrow kernels (bq_attn_fwd_pair): 1..32 queries, more than 128 keys"""
    return qa.shape[1] <= 32 and qb.shape[1] <= 32 and ka.shape[1] > 128 and kb.shape[1] > 128 and qa.shape[0] == qb.shape[0]


def _side(d, q, k, v, lse, mask_log2, seed):
    if k.stride() != v.stride():
        raise RuntimeError("attn pair: k and v must have equal strides")
    d.Q, d.K, d.V, d.LSE, d.mask = _p(q), _p(k), _p(v), _p(lse), _p(mask_log2)
    d.Lq, d.Lk, d.Lkp = q.shape[1], k.shape[1], _pad64(k.shape[1])
    (d.q_bs, d.q_rs, d.q_hs), (d.k_bs, d.k_rs, d.k_hs) = _bhd_strides(q), _bhd_strides(k)
    d.seed = int(seed) & 0xFFFFFFFF


def attn_fwd_pair(sides, scale, p_drop=0.0, seed_tensor=None):
    """two narrow attentions in one launch.  sides: two dicts with q (B, Lq <= 32, H, 64), k / v (B, Lk > 128, H, 64), out
    (B, Lq, H, 64) contiguous bf16 (written), mask_log2 (from key_mask_log2) or None, seed.  Returns the two lse (B, H, Lq)."""
    arr = (_AttnSide * 2)()
    q0 = sides[0]["q"]
    B, H = q0.shape[0], q0.shape[2]
    lses = []
    with torch.cuda.device(q0.device):
        for d, s in zip(arr, sides):
            q, out = s["q"], s["out"]
            if not q.is_cuda or out.shape != q.shape or out.dtype != torch.bfloat16 or not out.is_contiguous():
                raise RuntimeError("attn_fwd_pair: out must be a contiguous bf16 tensor shaped like q (CUDA)")
            lse = torch.empty(B, H, q.shape[1], dtype=torch.float32, device=q.device)
            _side(d, q, s["k"], s["v"], lse, s.get("mask_log2"), s.get("seed", 0))
            d.out = _p(out)
            d.o_bs, d.o_rs, d.o_hs = _bhd_strides(out)
            lses.append(lse)
        _check(_lib.bq_attn_fwd_pair(arr, B, H, float(scale), float(p_drop), _p(seed_tensor), _stream()), "attn_fwd_pair")
    return lses


def attn_bwd_pair(sides, scale, p_drop=0.0, seed_tensor=None):
    """backward of attn_fwd_pair.  sides: q, k, v, out (the forward's, contiguous), lse, grad_out, dq, dk, dv
    (preallocated bf16 views strided like q / k), mask_log2, seed."""
    arr = (_AttnSide * 2)()
    q0 = sides[0]["q"]
    B, H = q0.shape[0], q0.shape[2]
    keep = []
    with torch.cuda.device(q0.device):
        for d, s in zip(arr, sides):
            q, k, go = s["q"], s["k"], s["grad_out"]
            if s["dq"].stride() != q.stride() or s["dk"].stride() != k.stride() or s["dv"].stride() != k.stride():
                raise RuntimeError("attn_bwd_pair: stride contract violated")
            if go.stride(3) != 1 or go.stride(1) % 8 or go.stride(2) % 8:
                go = go.contiguous()
            if not s["out"].is_contiguous():
                raise RuntimeError("attn_bwd_pair: the forward output must be contiguous")
            delta = torch.empty(B, H, q.shape[1], dtype=torch.float32, device=q.device)
            keep += [go, delta]
            _side(d, q, k, s["v"], s["lse"], s.get("mask_log2"), s.get("seed", 0))
            d.dO, d.O, d.DELTA = _p(go), _p(s["out"]), _p(delta)
            d.out, d.dK, d.dV = _p(s["dq"]), _p(s["dk"]), _p(s["dv"])
            d.o_bs, d.o_rs, d.o_hs = _bhd_strides(go)
        _check(_lib.bq_attn_bwd_pair(arr, B, H, float(scale), float(p_drop), _p(seed_tensor), _stream()), "attn_bwd_pair")


def key_mask_log2_two(mask, B, Lk1, Lk2):
    """additive key mask broadcastable to (B,1,1,Lk1+Lk2) over cat(segment 1, segment 2) -> f32 (B, pad64(Lk1) +
    pad64(Lk2)) in the two-segment layout of bq_attn_fwd2 (each segment padded to a multiple of 64), times log2(e)"""
    if mask is None:
        return None
    p1 = _pad64(Lk1)
    m = torch.zeros(B, p1 + _pad64(Lk2), dtype=torch.float32, device=mask.device)
    src = mask.reshape(-1, Lk1 + Lk2).expand(B, Lk1 + Lk2).float() * LOG2E
    m[:, :Lk1] = src[:, :Lk1]
    m[:, p1:p1 + Lk2] = src[:, Lk1:]
    return m


def attn_fwd2(q, k1, v1, k2, v2, scale, mask_log2=None, p_drop=0.0, seed=0, seed_tensor=None, out=None):
    """attn_fwd over the keys cat(k1, k2) / values cat(v1, v2) without forming them (Lq <= 32).  k1 / v1 (B, Lk1, H, 64)
    views with equal strides, k2 / v2 (B, Lk2, H, 64) likewise; mask_log2 from key_mask_log2_two."""
    for t, n in ((q, "q"), (k1, "k1"), (v1, "v1"), (k2, "k2"), (v2, "v2")):
        if not t.is_cuda:
            raise RuntimeError("%s: CPU not supported" % n)
    if k1.stride() != v1.stride() or k2.stride() != v2.stride():
        raise RuntimeError("attn_fwd2: k and v of a segment must have equal strides")
    B, Lq, H, D = q.shape
    Lk1, Lk2 = k1.shape[1], k2.shape[1]
    Lkp = _pad64(Lk1) + _pad64(Lk2)
    with torch.cuda.device(q.device):
        if out is None:
            out = torch.empty(B, Lq, H, D, dtype=torch.bfloat16, device=q.device)
        elif out.shape != (B, Lq, H, D) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise RuntimeError("attn_fwd2: out must be a contiguous bf16 (B, Lq, H, 64) tensor")
        lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
        _check(_lib.bq_attn_fwd2(_p(q), _p(k1), _p(v1), _p(k2), _p(v2), _p(out), _p(lse), _p(mask_log2), B, H, Lq, Lk1,
                                 Lk2, Lkp, *_bhd_strides(q), *_bhd_strides(k1), *_bhd_strides(k2), *_bhd_strides(out),
                                 float(scale), float(p_drop), int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()),
               "attn_fwd2")
    return out, lse


def attn_bwd2(q, k1, v1, k2, v2, out, lse, grad_out, scale, dq, dk1, dv1, dk2, dv2, mask_log2=None, p_drop=0.0, seed=0,
              seed_tensor=None):
    """Backward of attn_fwd2.  dq strided like q, dk1 / dv1 like k1, dk2 / dv2 like k2 (preallocated bf16 views)."""
    B, Lq, H, D = q.shape
    Lk1, Lk2 = k1.shape[1], k2.shape[1]
    Lkp = _pad64(Lk1) + _pad64(Lk2)
    if (k1.stride() != v1.stride() or k2.stride() != v2.stride() or dq.stride() != q.stride() or
            dk1.stride() != k1.stride() or dv1.stride() != k1.stride() or dk2.stride() != k2.stride() or
            dv2.stride() != k2.stride()):
        raise RuntimeError("attn_bwd2: stride contract violated")
    with torch.cuda.device(q.device):
        if grad_out.stride(3) != 1 or grad_out.stride(1) % 8 or grad_out.stride(2) % 8:
            grad_out = grad_out.contiguous()
        if not out.is_contiguous():
            raise RuntimeError("attn_bwd2: the forward output must be contiguous")
        delta = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
        _check(_lib.bq_attn_bwd2(_p(q), _p(k1), _p(v1), _p(k2), _p(v2), _p(grad_out), _p(lse), _p(out), _p(delta),
                                 _p(mask_log2), _p(dq), _p(dk1), _p(dv1), _p(dk2), _p(dv2), B, H, Lq, Lk1, Lk2, Lkp,
                                 *_bhd_strides(q), *_bhd_strides(k1), *_bhd_strides(k2), *_bhd_strides(grad_out),
                                 float(scale), float(p_drop), int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()),
               "attn_bwd2")


_COLSUM_SLOTS = 1 << 16
_colsum_counters = {}
_colsum_next = [0]


def _colsum_counter(device, n):
    """n zeroed, self-resetting completion counters that no other in-flight colsum launch uses (rotating slots)"""
    key = device.index if device.index is not None else torch.cuda.current_device()
    pool = _colsum_counters.get(key)
    if pool is None:
        pool = _colsum_counters[key] = torch.zeros(_COLSUM_SLOTS, dtype=torch.int32, device=device)
    if _colsum_next[0] + n > _COLSUM_SLOTS:
        _colsum_next[0] = 0
    base = _colsum_next[0]
    _colsum_next[0] += n
    return pool.data_ptr() + 4 * base


def colsum(g2d):
    """f32 column sums of a contiguous bf16 (M, N) matrix (bias gradients), N % 4 == 0.  One launch."""
    M, N = g2d.shape
    with torch.cuda.device(g2d.device):
        out = torch.empty(N, dtype=torch.float32, device=g2d.device)
        chunks = _lib.bq_colsum_chunks(M)
        part = cnt = None
        if chunks > 1:
            part = torch.empty(chunks * N, dtype=torch.float32, device=g2d.device)
            cnt = _colsum_counter(g2d.device, (N + 255) // 256)
        _check(_lib.bq_colsum_bf16(_p(g2d), _p(out), M, N, _p(part), cnt, _stream()), "colsum")
    return out


def gelu_fwd(x):
    """exact GELU of a contiguous bf16 tensor (numel % 8 == 0)"""
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        _check(_lib.bq_gelu_fwd_bf16(_p(x), _p(y), x.numel(), _stream()), "gelu_fwd")
    return y


# ---- multi-tensor AdamW that also writes the bf16 shadows (csrc/adamw.hip) -----------------------------
ADAMW_CHUNK = _lib.bq_adamw_chunk_elems()
ADAMW_TENSOR_BYTES = _lib.bq_adamw_tensor_bytes()


def adamw_multi(table, chunks, step, beta1, beta2, eps, grad_clip_value=0.0):
    """table: uint8 device tensor of packed AdamWTensor records; chunks: int32 (n, 2) device tensor; step: f32 device
    scalar holding the 1-based count of THIS update; grad_clip_value > 0: gradients clamped to +-value as they are read."""
    with torch.cuda.device(table.device):
        _check(_lib.bq_adamw_multi(_p(table), _p(chunks), chunks.shape[0], _p(step), float(beta1), float(beta2),
                                   float(eps), float(grad_clip_value or 0.0), _stream()), "adamw")


# ---- multi-tensor bf16 transpose (csrc/transpose.hip): the K-contiguous copies of the text side's weights -------
TRANSPOSE_TENSOR_BYTES = _lib.bq_transpose_tensor_bytes()


def transpose_table(pairs, device):
    """pairs: [(src (N, K) bf16 with a contiguous last dim, dst (K, N) bf16 contiguous)], N and K multiples of 64 ->
    (table, chunks) device tensors for transpose_multi"""
    import struct
    assert TRANSPOSE_TENSOR_BYTES == 32
    rec, chunks = [], []
    for i, (src, dst) in enumerate(pairs):
        N, K = src.shape
        if (src.dtype != torch.bfloat16 or dst.dtype != torch.bfloat16 or src.stride(1) != 1 or not dst.is_contiguous()
                or tuple(dst.shape) != (K, N) or N % 64 or K % 64 or src.stride(0) % 8 or src.data_ptr() % 16
                or dst.data_ptr() % 16):
            raise RuntimeError("transpose_table: unsupported pair %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
        rec.append(struct.pack("<QQiiii", src.data_ptr(), dst.data_ptr(), N, K, src.stride(0), K // 64))
        chunks.append(torch.stack([torch.full((N // 64 * (K // 64),), i, dtype=torch.int32),
                                   torch.arange(N // 64 * (K // 64), dtype=torch.int32)], dim=1))
    table = torch.frombuffer(bytearray(b"".join(rec)), dtype=torch.uint8).to(device)
    return table, torch.cat(chunks, dim=0).contiguous().to(device)


def transpose_multi(table, chunks, max_wgs=0):
    """max_wgs > 0: at most that many workgroups walk the tiles (beside a latency-bound chain); 0: one per tile"""
    with torch.cuda.device(table.device):
        _check(_lib.bq_transpose_multi_bf16(_p(table), _p(chunks), chunks.shape[0], int(max_wgs), _stream()), "transpose_multi")


# ---- training-mode BatchNorm + ReLU (+ max over nsample) on point-major bf16 rows (csrc/bn.hip) -------


def bn_relu_fwd(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, S, relu, pool):
    """x: bf16 (R, C) contiguous rows (point-major activations).  Batch statistics (running buffers updated in
    place), then y = relu?(bn(x)) as bf16 (R, C), or (R // S, C) = max over every run of S rows when pool.
    Returns y and the saved statistics (scale, shift, mean, rstd: one f32 (4, C) tensor)."""
    if not x.is_cuda:
        raise RuntimeError("x: CPU not supported")
    R, C = x.shape
    with torch.cuda.device(x.device):
        stats = torch.empty(4, C, dtype=torch.float32, device=x.device)
        part = torch.empty(_lib.bq_bn_chunks(R, 0, 0) * 2 * C, dtype=torch.float32, device=x.device)
        _check(_lib.bq_bn_stats(_p(x), R, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                _p(num_batches_tracked), float(eps), float(momentum), _p(part), _p(stats[0]),
                                _p(stats[1]), _p(stats[2]), _p(stats[3]), _stream()), "bn_stats")
        y = torch.empty(R // S if pool else R, C, dtype=torch.bfloat16, device=x.device)
        _check(_lib.bq_bn_apply(_p(x), _p(stats[0]), _p(stats[1]), _p(y), R, C, int(S), int(bool(relu)),
                                int(bool(pool)), _stream()), "bn_apply")
    return y, stats


def bn_relu_bwd(dy, x, stats, S, relu, pool):
    """-> dx bf16 (R, C), dgamma f32 (C), dbeta f32 (C)"""
    R, C = x.shape
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
        part = torch.empty(_lib.bq_bn_chunks(R, int(S), int(bool(pool))) * 2 * C, dtype=torch.float32, device=x.device)
        _check(_lib.bq_bn_backward(_p(dy), _p(x), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(part),
                                   _p(dgb), _p(dx), R, C, int(S), int(bool(relu)), int(bool(pool)), _stream()),
               "bn_backward")
    return dx, dgb[1], dgb[0]


# ---- fused dropout + residual + LayerNorm (csrc/ln.hip) ---------------------------------------------
def drop_add_ln_fwd(x, residual, gamma, beta, eps, p_drop, seed, seed_tensor, want_sum=False, p_path=0.0,
                    rows_per_sample=0, want_dgb=False):
    """y = LayerNorm(path(dropout(x)) + residual); x, residual bf16 (..., H) contiguous, residual may be None;
    path = stochastic depth per sample of rows_per_sample rows (p_path = 0: identity).
    Returns y, sum (the bf16 pre-norm sum, or None unless want_sum), mean, rstd, dgb (zeroed f32 (2, H) accumulator
    for drop_add_ln_bwd, or None unless want_dgb)."""
    H = x.shape[-1]
    M = x.numel() // H
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        s = torch.empty_like(x) if want_sum else None
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
        dgb = torch.empty(2, H, dtype=torch.float32, device=x.device) if want_dgb else None
        _check(_lib.bq_drop_add_ln_fwd(_p(x), _p(residual), _p(gamma), _p(beta), _p(y), _p(s), _p(mean), _p(rstd),
                                       _p(dgb), M, H, float(eps), float(p_drop), float(p_path), int(rows_per_sample),
                                       int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()), "drop_add_ln_fwd")
    return y, s, mean, rstd, dgb


def drop_add_ln_bwd(x, residual, gamma, dy, mean, rstd, eps, p_drop, seed, seed_tensor, dsum=None, p_path=0.0,
                    rows_per_sample=0, dgb=None):
    """-> dx, dresidual (None when residual is None), dgamma, dbeta; dsum = gradient of the `sum` output; dgb = the
    zeroed accumulator the forward handed out (a fresh zeros(2, H) when None)"""
    H = x.shape[-1]
    M = x.numel() // H
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if residual is not None else None
        if dgb is None:
            dgb = torch.zeros(2, H, dtype=torch.float32, device=x.device)
        if _det():
            _ln_bwd_det(x, residual, gamma, None, 1, dy, dsum, mean, rstd, dx, dres, dgb, M, H, eps, p_drop, p_path,
                        rows_per_sample, seed, seed_tensor, 0, "drop_add_ln_bwd_det")
            return dx, dres, dgb[0], dgb[1]
        _check(_lib.bq_drop_add_ln_bwd(_p(x), _p(residual), _p(gamma), _p(dy), _p(dsum), _p(mean), _p(rstd), _p(dx),
                                       _p(dres), _p(dgb), M, H, float(eps), float(p_drop), float(p_path),
                                       int(rows_per_sample), int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()),
               "drop_add_ln_bwd")
    return dx, dres, dgb[0], dgb[1]


def drop_add_ln_bwd_sum(s, gamma, dy, mean, rstd, eps, seed, seed_tensor, dsum=None, p_path=0.0, rows_per_sample=0, dgb=None):
    """the backward of a dropout-free site from its stored sum `s` (include/bqhip_fusion.h: bq_drop_add_ln_bwd_sum)
    -> dx, dresidual (the SAME tensor as dx when p_path == 0), dgamma, dbeta"""
    H = s.shape[-1]
    M = s.numel() // H
    with torch.cuda.device(s.device):
        dx = torch.empty_like(s)
        dres = torch.empty_like(s) if p_path > 0 else None
        if dgb is None:
            dgb = torch.zeros(2, H, dtype=torch.float32, device=s.device)
        if _det():
            _ln_bwd_det(s, None, gamma, None, 1, dy, dsum, mean, rstd, dx, dres, dgb, M, H, eps, 0.0, p_path, rows_per_sample,
                        seed, seed_tensor, 1, "drop_add_ln_bwd_sum_det")
            return dx, (dres if dres is not None else dx), dgb[0], dgb[1]
        _check(_lib.bq_drop_add_ln_bwd_sum(_p(s), _p(gamma), _p(dy), _p(dsum), _p(mean), _p(rstd), _p(dx), _p(dres), _p(dgb),
                                           M, H, float(eps), float(p_path), int(rows_per_sample), int(seed) & 0xFFFFFFFF,
                                           _p(seed_tensor), _stream()), "drop_add_ln_bwd_sum")
    return dx, (dres if dres is not None else dx), dgb[0], dgb[1]


def twin_drop_add_ln_fwd(x, residual, gamma, beta, gamma2, beta2, eps, p_drop, seed, seed_tensor, want_dgb=False):
    """drop_add_ln_fwd over two row groups (first / second half of the rows of x) with their own LayerNorm parameters;
    returns y, mean, rstd, dgb (zeroed f32 (2, 2, H), or None)"""
    H = x.shape[-1]
    M = x.numel() // H
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
        dgb = torch.empty(2, 2, H, dtype=torch.float32, device=x.device) if want_dgb else None
        _check(_lib.bq_twin_drop_add_ln_fwd(_p(x), _p(residual), _p(gamma), _p(beta), _p(gamma2), _p(beta2), _p(y),
                                            _p(mean), _p(rstd), _p(dgb), M, H, float(eps), float(p_drop),
                                            int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()), "twin_drop_add_ln_fwd")
    return y, mean, rstd, dgb


def twin_drop_add_ln_bwd(x, residual, gamma, gamma2, dy, mean, rstd, eps, p_drop, seed, seed_tensor, dgb=None):
    """-> dx, dresidual, dgb (2, 2, H): [group][dgamma | dbeta]"""
    H = x.shape[-1]
    M = x.numel() // H
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if residual is not None else None
        if dgb is None:
            dgb = torch.zeros(2, 2, H, dtype=torch.float32, device=x.device)
        if _det():
            _ln_bwd_det(x, residual, gamma, gamma2, 2, dy, None, mean, rstd, dx, dres, dgb, M, H, eps, p_drop, 0.0, 0, seed,
                        seed_tensor, 0, "twin_drop_add_ln_bwd_det")
            return dx, dres, dgb
        _check(_lib.bq_twin_drop_add_ln_bwd(_p(x), _p(residual), _p(gamma), _p(gamma2), _p(dy), _p(mean), _p(rstd),
                                            _p(dx), _p(dres), _p(dgb), M, H, float(eps), float(p_drop),
                                            int(seed) & 0xFFFFFFFF, _p(seed_tensor), _stream()), "twin_drop_add_ln_bwd")
    return dx, dres, dgb


# ---- proposal post-processing (csrc/nms.hip) ------------------------------------------------------------


def box_point_count(points, center, size, heading, cap=0):
    """points f32 (B, N, >=3) (xyz first), center / size f32 (B, K, 3), heading f32 (B, K) -> i32 (B, K) points inside each
    oriented box (closed)"""
    for t, n in ((points, "points"), (center, "center"), (size, "size"), (heading, "heading")):
        if not t.is_cuda:
            raise RuntimeError("%s: CPU not supported" % n)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous float32 tensor" % n)
    B, N, ld = points.shape
    K = center.shape[1]
    with torch.cuda.device(points.device):
        out = torch.empty(B, K, dtype=torch.int32, device=points.device)
        _check(_lib.bq_box_point_count(_p(points), _p(center), _p(size), _p(heading), _p(out), B, N, ld, K, int(cap),
                                       _stream()), "box_point_count")
    return out


def nms(box, score, thresh, cls=None, valid=None, old_type=False, same_cls=False):
    """box f32 (B, K, 6) axis-aligned extents, score f32 (B, K), cls i32 (B, K), valid u8 / bool (B, K) -> bool (B, K);
    thresh is compared as the Python float (a double), NaN scores are visited first, ties in index order"""
    if not box.is_cuda:
        raise RuntimeError("box: CPU not supported")
    B, K = score.shape
    box, score = box.contiguous().float(), score.contiguous().float()
    cls = cls.contiguous().to(torch.int32) if cls is not None else None
    valid = valid.contiguous().to(torch.uint8) if valid is not None else None
    with torch.cuda.device(box.device):
        keep = torch.empty(B, K, dtype=torch.uint8, device=box.device)
        _check(_lib.bq_nms_f64(_p(box), _p(score), _p(cls), _p(valid), _p(keep), B, K, float(thresh), int(bool(old_type)),
                               int(bool(same_cls)), _stream()), "nms")
    return keep.bool()


# ---- detection mAP (csrc/ap_eval.hip) --------------------------------------------------------------------
_d = ctypes.c_double


def _ap_req(t, dtype, shape_tail, name):
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported" % name)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape[1:]) != shape_tail:
        raise RuntimeError("%s must be a contiguous %s tensor of shape (n%s)" % (name, dtype, "".join(", %d" % s for s in shape_tail)))


def ap_match(box_tab, det_box, gt_tab, seg_det, seg_gt, thresholds, max_seg_gt=None):
    """box_tab f64 (Nb, 6), det_box i32 (D), gt_tab f64 (G, 6), seg_det / seg_gt i32 (S + 1) CSR offsets, thresholds: up to
    4 floats -> tp u8 (T, D), ovmax f64 (D), jmax i32 (D).  max_seg_gt: the largest segment's ground-truth count when the
    caller knows a bound (no synchronisation); None reads it from seg_gt (one device -> host copy)."""
    _ap_req(box_tab, torch.float64, (6,), "box_tab")
    _ap_req(det_box, torch.int32, (), "det_box")
    _ap_req(gt_tab, torch.float64, (6,), "gt_tab")
    _ap_req(seg_det, torch.int32, (), "seg_det")
    _ap_req(seg_gt, torch.int32, (), "seg_gt")
    if seg_det.numel() != seg_gt.numel() or seg_det.numel() < 1:
        raise RuntimeError("ap_match: seg_det %d and seg_gt %d offsets" % (seg_det.numel(), seg_gt.numel()))
    thr = [float(t) for t in thresholds]
    T, D, S = len(thr), det_box.numel(), seg_det.numel() - 1
    if max_seg_gt is None:
        max_seg_gt = int((seg_gt[1:] - seg_gt[:-1]).max().item()) if S > 0 else 0
    with torch.cuda.device(box_tab.device):
        dev = box_tab.device
        tp = torch.zeros(max(T, 1), D, dtype=torch.uint8, device=dev)
        ovmax = torch.full((D,), float("-inf"), dtype=torch.float64, device=dev)
        jmax = torch.full((D,), -1, dtype=torch.int32, device=dev)
        _check(_lib.bq_ap_match(_p(box_tab), _p(det_box), _p(gt_tab), _p(seg_det), _p(seg_gt), (_d * max(T, 1))(*thr),
                                _p(tp), _p(ovmax), _p(jmax), box_tab.shape[0], D, gt_tab.shape[0], S, T, int(max_seg_gt),
                                _stream()), "ap_match")
    return tp, ovmax, jmax


def ap_curve(tp, cls_off, npos):
    """tp u8 (T, D) in curve order, cls_off i32 (C + 1), npos f64 (C) -> rec, prec f64 (T, D), ap, last_recall f64 (C, T)"""
    if tp.dim() != 2:
        raise RuntimeError("tp must be (T, D)")
    _ap_req(tp, torch.uint8, (tp.shape[1],), "tp")
    _ap_req(cls_off, torch.int32, (), "cls_off")
    _ap_req(npos, torch.float64, (), "npos")
    T, D = tp.shape
    C = npos.numel()
    if cls_off.numel() != C + 1:
        raise RuntimeError("ap_curve: %d class offsets for %d classes" % (cls_off.numel(), C))
    with torch.cuda.device(tp.device):
        rec = torch.zeros(T, D, dtype=torch.float64, device=tp.device)
        prec = torch.zeros(T, D, dtype=torch.float64, device=tp.device)
        ap = torch.zeros(C, T, dtype=torch.float64, device=tp.device)
        last = torch.zeros(C, T, dtype=torch.float64, device=tp.device)
        _check(_lib.bq_ap_curve(_p(tp), _p(cls_off), _p(npos), _p(rec), _p(prec), _p(ap), _p(last), D, C, T, _stream()),
               "ap_curve")
    return rec, prec, ap, last


# ---- multiview projection (csrc/projection.hip) ---------------------------------------------------------


def project_points(points, depth, frames, image_dims, fx, fy, cx, cy, depth_min, depth_max, accuracy):
    """points f32 (N, 3), depth f32 (F, H, W), frames f32 (F, 40) -> i32 (F, N): pixel index y * W + x or -1"""
    for t, n in ((points, "points"), (depth, "depth"), (frames, "frames")):
        if not t.is_cuda:
            raise RuntimeError("%s: CPU not supported" % n)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous float32 tensor" % n)
    W, H = int(image_dims[0]), int(image_dims[1])
    F, N = depth.shape[0], points.shape[0]
    if depth.numel() != F * W * H or frames.shape != (F, 40) or points.shape[1] != 3:
        raise RuntimeError("project_points: shapes %s %s %s" % (tuple(points.shape), tuple(depth.shape), tuple(frames.shape)))
    with torch.cuda.device(points.device):
        pix = torch.empty(F, N, dtype=torch.int32, device=points.device)
        _check(_lib.bq_project_points(_p(points), _p(depth), _p(frames), _p(pix), F, N, W, H, float(fx), float(fy), float(cx),
                                      float(cy), float(depth_min), float(depth_max), float(accuracy), _stream()),
               "project_points")
    return pix


def fuse_point_features(pix, feat, maxpool):
    """pix i32 (F, N), feat f32 (F, H*W, C) pixel-major -> f32 (N, C)"""
    if not (pix.is_cuda and feat.is_cuda):
        raise RuntimeError("fuse_point_features: CPU not supported")
    if pix.dtype != torch.int32 or feat.dtype != torch.float32 or not pix.is_contiguous() or not feat.is_contiguous():
        raise RuntimeError("fuse_point_features: pix must be contiguous int32, feat contiguous float32")
    F, N = pix.shape
    if feat.dim() != 3 or feat.shape[0] != F:
        raise RuntimeError("fuse_point_features: feat must be (F, H*W, C)")
    HW, C = feat.shape[1], feat.shape[2]
    with torch.cuda.device(pix.device):
        out = torch.empty(N, C, dtype=torch.float32, device=pix.device)
        _check(_lib.bq_fuse_point_features(_p(pix), _p(feat), _p(out), F, N, HW, C, int(bool(maxpool)), _stream()),
               "fuse_point_features")
    return out


# ---- MFMA bf16 GEMM family (csrc/gemm.hip) ------------------------------------------------------------
GEMM_P_XC, GEMM_Q_XC, GEMM_OUT_F32, GEMM_BACKGROUND = (_D["BQ_GEMM_" + n] for n in ("P_XC", "Q_XC", "OUT_F32", "BACKGROUND"))
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_BIAS_CE, EPI_ADD = (
    _D["BQ_GEMM_EPI_" + n] for n in ("NONE", "BIAS", "BIAS_GELU", "DGELU", "BIAS_CE", "ADD"))
GEMM_DET = _D["BQ_GEMM_DET"]   # set by gemm_grouped itself in the deterministic mode
GEMM_SECOND = _D["BQ_GEMM_SECOND"]   # set by gemm_grouped itself when a problem carries P2 / Q2
_GemmDesc = _cabi.STRUCTS["bq_gemm_desc"]


def _mat(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported (bridgeqa_amd has no CPU path)" % name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError("%s must be a 2-D tensor with a contiguous last dimension" % name)
    return t


def _mat_rows(t, name):
    """Q / out / aux / out2 of a GEMM problem: a 2-D (rows, cols) tensor, or a 3-D (batch, rows_per_batch, cols) VIEW whose
    batches are stride(0) elements apart -- the batched-row map of bq_gemm_desc (q_rpb / o_rpb), e.g. kv[:, :1025] of a
    (B, 1045, 1536) key/value tensor.  Returns (shape2d, ld, rpb, bstride); a 3-D tensor that is plain rows comes back
    with rpb = 0."""
    if not t.is_cuda:
        raise RuntimeError("%s: CPU not supported (bridgeqa_amd has no CPU path)" % name)
    if t.dim() == 2:
        if t.stride(1) != 1:
            raise RuntimeError("%s must have a contiguous last dimension" % name)
        return (t.shape[0], t.shape[1]), t.stride(0), 0, 0
    if t.dim() != 3 or t.stride(2) != 1:
        raise RuntimeError("%s must be (rows, cols) or a (batch, rows, cols) view with a contiguous last dimension" % name)
    B, R, C = t.shape
    ld, bs = t.stride(1), t.stride(0)
    if B == 1 or bs == R * ld:
        return (B * R, C), ld, 0, 0
    if bs < R * ld or bs % 8 or R > 65535:
        raise RuntimeError("%s: unsupported batched-row view (stride %s, shape %s)" % (name, t.stride(), tuple(t.shape)))
    return (B * R, C), ld, R, bs


def gemm_grouped(problems, flags, epilogue=EPI_NONE, tile=None, fixed_order=False):
    """One launch for a list of problems out[j][i] = epilogue(sum_kc P(i,kc) Q(j,kc)) (include/bqhip_fusion.h,
    bq_gemm_bf16).  problems: dicts with P, Q, out (2-D tensors, contiguous last dim) and optional bias (fp32 (Ni,)),
    out2, aux, colsum (fp32 (Ni,), accumulated).  P: (Ni, Kc), or (Kc, Ni) with GEMM_P_XC; Q likewise over j.
    P2 / Q2 (weight-gradient form on tile 256 only): a second row source, out = Q^T P + Q2^T P2 in the same launch (BQ_GEMM_SECOND;
    Q2 may be a batched-row view of any rows per batch); such a problem takes two of the launch's bq_gemm_max_problems() entries.
    fixed_order: take the deterministic mode's form (a cut contraction summed in piece order instead of with fp32 atomics)
    for this launch whatever the mode -- for results that feed further backward passes."""
    if _det() or fixed_order:
        return _gemm_grouped_det(problems, flags, epilogue, tile)
    return _gemm_grouped_launch(problems, flags, epilogue, tile)


def _gemm_pack(d, pr, flags, epilogue):
    """validate one problem dict and fill its bq_gemm_desc `d`; returns what the tile policy reads of it (gemm_route.Shape)"""
    pxc, qxc, f32 = bool(flags & GEMM_P_XC), bool(flags & GEMM_Q_XC), bool(flags & GEMM_OUT_F32)
    P, Q, out = _mat(pr["P"], "P"), pr["Q"], pr["out"]
    qshape, ldq, q_rpb, q_bs = _mat_rows(Q, "Q")
    oshape, ldo, o_rpb, o_bs = _mat_rows(out, "out")
    if P.dtype != torch.bfloat16 or Q.dtype != torch.bfloat16:
        raise RuntimeError("gemm: operands must be bf16")
    if out.dtype != (torch.float32 if f32 else torch.bfloat16):
        raise RuntimeError("gemm: out must be %s" % ("float32" if f32 else "bfloat16"))
    Ni, Kc = (P.shape[1], P.shape[0]) if pxc else (P.shape[0], P.shape[1])
    Nj, Kq = (qshape[1], qshape[0]) if qxc else (qshape[0], qshape[1])
    Ni = int(pr.get("Ni", Ni))  # output wider than P's rows (padded vocabulary): P's true extent goes in p_bytes
    if (Kq != Kc and "Kc" not in pr) or tuple(oshape) != (Nj, Ni):
        raise RuntimeError("gemm: shape mismatch P%s Q%s out%s" % (tuple(P.shape), tuple(Q.shape), tuple(out.shape)))
    d.P, d.Q, d.out = P.data_ptr(), Q.data_ptr(), out.data_ptr()
    bias, out2, aux, colsum = pr.get("bias"), pr.get("out2"), pr.get("aux"), pr.get("colsum")
    if bias is not None and (bias.dtype not in (torch.float32, torch.bfloat16) or bias.numel() != Ni
                             or not bias.is_contiguous()):
        raise RuntimeError("gemm: bias must be a contiguous fp32 or bf16 (Ni,) tensor")
    d.bias_bf16 = int(bias is not None and bias.dtype == torch.bfloat16)
    # (weight-gradient form: colsum (Nj,) receives the column sums of Q over the contraction; with ksplit > 1 it is
    # accumulated with atomics and must arrive zeroed)
    n_cs = Nj if (pxc and qxc and f32) else Ni
    if epilogue != EPI_BIAS_CE and colsum is not None and (colsum.dtype != torch.float32 or colsum.numel() != n_cs
                                                           or not colsum.is_contiguous()):
        raise RuntimeError("gemm: colsum must be a contiguous fp32 (%d,) tensor" % n_cs)
    for t, nm in ((out2, "out2"), (aux, "aux")):
        if epilogue != EPI_BIAS_CE and t is not None and (t.dtype != torch.bfloat16 or t.shape != out.shape
                                                          or t.stride() != out.stride()):
            raise RuntimeError("gemm: %s must be bf16 and laid out like out" % nm)
    d.bias, d.out2, d.aux, d.colsum = _p(bias), _p(out2), _p(aux), _p(colsum)
    d.ldp, d.ldq, d.ldo = P.stride(0), ldq, ldo
    d.q_rpb, d.q_bstride, d.o_rpb, d.o_bstride = q_rpb, q_bs, o_rpb, o_bs
    d.accum = int(bool(pr.get("accum", False)))
    # (Kc given: a contraction longer than the K-contiguous operand's rows -- its partner is zero-padded)
    d.Ni, d.Nj, d.Kc = Ni, Nj, int(pr.get("Kc", Kc))
    d.p_bytes, d.q_bytes, d.ksplit = int(pr.get("p_bytes", 0)), int(pr.get("q_bytes", 0)), int(pr.get("ksplit", 1))
    return gemm_route.Shape(Ni, Nj, d.Kc, colsum is not None, bool(q_rpb or o_rpb))


def _gemm_pack_second(d, pr, prim):
    """the second row source of a weight gradient (problem keys P2 / Q2: dW = Q^T P + Q2^T P2 in one pass, BQ_GEMM_SECOND) as
    the array entry behind its primary `prim`: no out.  The library checks the form, the tile and the extents."""
    if pr.get("P2") is None or pr.get("Q2") is None:
        raise RuntimeError("gemm: a second row source needs both P2 and Q2")
    P2, Q2 = _mat(pr["P2"], "P2"), pr["Q2"]
    qshape, ldq, q_rpb, q_bs = _mat_rows(Q2, "Q2")
    if P2.dtype != torch.bfloat16 or Q2.dtype != torch.bfloat16:
        raise RuntimeError("gemm: operands must be bf16")
    if P2.shape[0] != qshape[0] or P2.shape[1] != prim.Ni or qshape[1] != prim.Nj:
        raise RuntimeError("gemm: shape mismatch P2%s Q2%s for a (%d, %d) weight gradient" % (
            tuple(P2.shape), tuple(Q2.shape), prim.Nj, prim.Ni))
    d.P, d.Q = P2.data_ptr(), Q2.data_ptr()
    d.ldp, d.ldq, d.q_rpb, d.q_bstride = P2.stride(0), ldq, q_rpb, q_bs
    d.Ni, d.Nj, d.Kc, d.ksplit = prim.Ni, prim.Nj, P2.shape[0], 1


def _gemm_grouped_launch(problems, flags, epilogue, tile):
    two = [("P2" in pr) or ("Q2" in pr) for pr in problems]
    n = len(problems) + sum(two)
    arr = (_GemmDesc * n)()
    shapes, k = [], 0
    for pr, second in zip(problems, two):
        shapes.append(_gemm_pack(arr[k], pr, flags, epilogue))
        k += 1
        if second:
            _gemm_pack_second(arr[k], pr, arr[k - 1])
            k += 1
    if any(two):
        flags |= GEMM_SECOND
    tile = int(tile or gemm_route.auto_tile(shapes, flags, epilogue))
    dev = problems[0]["out"].device
    if tile != 128:
        flags &= ~GEMM_BACKGROUND   # (only the persistent 256 x 128 kernel has a reduced grid)
    with torch.cuda.device(dev):
        if tile == 128 and n == 1 and (STREAMK[0] or STREAMK256[0]):
            _streamk_workspace(dev)
        _check(_lib.bq_gemm_bf16(arr, n, int(flags), int(epilogue), tile, _stream()), "gemm_bf16")


def _gemm_grouped_det(problems, flags, epilogue, tile):
    """gemm_grouped in its fixed-order form (DET_ROUTES) -- every launch of the deterministic mode, and in any mode a launch
    that asks for it (gemm_grouped(fixed_order=True): the LM head's dH): the launch carries GEMM_DET; a cut fp32 contraction
    (ksplit > 1) runs into per-piece slabs that bq_gemm_splitk_fold_det adds onto `out` in piece order; column sums of a bf16
    output are taken after the launch by the grouped fixed-order column sum.  Refuses what has no fixed-order form: a cut
    contraction with column sums and, while the deterministic mode is on, stream-K (a whole step must not mix the two; a single
    fixed-order launch beside stream-K in the default mode is fine -- stream-K lives in the large-tile kernels, the fixed-order
    forms in the small-tile one, and the library refuses GEMM_DET on the one tile class where they could meet)."""
    if _det() and (STREAMK[0] or STREAMK256[0]):
        raise RuntimeError("gemm: stream-K is on (streamk_enable / streamk256_enable) while the deterministic mode is on")
    f32 = bool(flags & GEMM_OUT_F32)
    probs, folds, sums = [], [], []
    for pr in problems:
        ks = int(pr.get("ksplit", 1))
        if epilogue != EPI_BIAS_CE and ks > 1:
            out = pr["out"]
            if not f32 or pr.get("colsum") is not None or pr.get("accum") or out.dim() != 2 or out.stride(1) != 1:
                raise RuntimeError("gemm: a cut contraction in the deterministic mode needs fp32 plain-row out, no colsum or accum")
            slab = torch.empty(ks, out.shape[0], out.stride(0), dtype=torch.float32, device=out.device)
            folds.append((slab, out, ks))
            pr = dict(pr, out=slab[0, :, :out.shape[1]])
        elif not f32 and epilogue != EPI_BIAS_CE and pr.get("colsum") is not None:
            sums.append((pr["out"], pr["colsum"]))
            pr = dict(pr, colsum=None)
        probs.append(pr)
    _gemm_grouped_launch(probs, flags | GEMM_DET, epilogue, tile)
    for slab, out, ks in folds:
        R, C = out.shape
        with torch.cuda.device(out.device):
            _check(_det_entry("gemm_splitk_fold")(_p(slab), _p(out), None, ks, R, C, out.stride(0), _stream()),
                   "gemm_splitk_fold_det")
    if sums:
        _colsum_grouped_into([o.reshape(-1, o.shape[-1]) if o.dim() == 3 else o for o, _ in sums], [c for _, c in sums],
                             "gemm_epilogue_colsum")


# ---- stream-K workspaces (bq_gemm_set_workspace): one per (device, stream), allocated at the first tile-128 single-problem
# launch on that stream OUTSIDE a capture (the warm-up steps of pipeline.py / graphed.py run on the phase streams first); a
# launch on a stream without one runs on whole tiles
STREAMK = [False]   # the 256 x 128 kernel's stream-K form: built, parity-green, SLOWER on every shape measured
# the 256 x 256 kernel's stream-K form (the vendor library's design for these shapes): built at the end of round 5, parity-green,
# SLOWER too (fc2 forward 98.6 us against 76.7 on whole 256 x 256 tiles and 75.4 on 256 x 128; c3 + 0.9 ms) -- off;
# BQ_GEMM_STREAMK256=1 switches it on
STREAMK256 = [os.environ.get("BQ_GEMM_STREAMK256", "0") == "1"]
_SK_WS = {}


def _streamk_apply():
    on = STREAMK[0] or STREAMK256[0]
    _lib.bq_gemm_streamk_mode((1 if STREAMK[0] else 0) | (2 if STREAMK256[0] else 0))
    for (d, sp), (ws, st) in _SK_WS.items():
        with torch.cuda.device(d):
            _check(_lib.bq_gemm_set_workspace(_p(ws) if on else None, ws.numel() if on else 0, sp), "gemm_set_workspace")


def streamk_enable(flag):
    """measurement / test switch of the 256 x 128 kernel's stream-K form (with both forms off every registered workspace is
    withdrawn and the launches run on whole tiles)"""
    STREAMK[0] = bool(flag)
    _streamk_apply()


def streamk256_enable(flag):
    """the same for the 256 x 256 kernel's form (product default: off as well)"""
    STREAMK256[0] = bool(flag)
    _streamk_apply()


_streamk_apply()


def _streamk_workspace(dev):
    st = torch.cuda.current_stream(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), st.cuda_stream)
    if key in _SK_WS or torch.cuda.is_current_stream_capturing():
        return
    nbytes = int(_lib.bq_gemm_workspace_bytes())
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)     # (the tickets at its head must start at zero)
    _check(_lib.bq_gemm_set_workspace(_p(ws), nbytes, st.cuda_stream), "gemm_set_workspace")
    _SK_WS[key] = (ws, st)      # (the stream object is kept: its handle must not be recycled for another stream)


def gemm_fwd(x, w, bias=None, gelu=False, tile=None, out=None, background=False):
    """y = x @ w^T + bias (x (M,K), w (N,K) bf16; bias fp32 (N,)); gelu: returns (y_pre, gelu(y_pre)); out: write y there;
    background: GEMM_BACKGROUND (a side-stream launch that leaves room on every CU)"""
    _mat(x, "x"), _mat(w, "w")
    M, N = x.shape[0], w.shape[0]
    with torch.cuda.device(x.device):
        y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device) if out is None else out
        act = torch.empty_like(y) if gelu else None
    epi = EPI_BIAS_GELU if gelu else (EPI_BIAS if bias is not None else EPI_NONE)
    gemm_grouped([dict(P=w, Q=x, out=y, bias=bias, out2=act)], GEMM_BACKGROUND if background else 0, epi, tile)
    return (y, act) if gelu else y


def gemm_dx(dy, w, pre_act=None, colsum=None, tile=None, add=None, background=False, wt=None):
    """dx = dy @ w (dy (M,N), w (N,K) bf16) [* gelu'(pre_act) (M,K)] [+ add (M,K) bf16]; colsum (K,) fp32 += column
    sums of dx.  wt: w's transpose (K,N), contiguous -- the launch then reads it K-contiguous like a forward (the small-M
    launches of the text side: fusion_state.transposed_shadow) instead of walking w's rows contraction-major"""
    _mat(dy, "dy"), _mat(w, "w")
    M, K = dy.shape[0], w.shape[1]
    if pre_act is not None and add is not None:
        raise RuntimeError("gemm_dx: pre_act and add are exclusive")
    if wt is not None and (colsum is not None or tuple(wt.shape) != (K, w.shape[0])):
        wt = None
    with torch.cuda.device(dy.device):
        dx = torch.empty(M, K, dtype=torch.bfloat16, device=dy.device)
    gemm_grouped([dict(P=w if wt is None else wt, Q=dy, out=dx, aux=pre_act if add is None else add, colsum=colsum)],
                 (GEMM_P_XC if wt is None else 0) | (GEMM_BACKGROUND if background else 0),
                 EPI_DGELU if pre_act is not None else (EPI_ADD if add is not None else EPI_NONE), tile)
    return dx


def gemm_dw(dy, x, tile=None):
    """dw = dy^T @ x in fp32 (dy (M,N), x (M,K) bf16) -> (N,K)"""
    _mat(dy, "dy"), _mat(x, "x")
    N, K = dy.shape[1], x.shape[1]
    with torch.cuda.device(dy.device):
        dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
    gemm_grouped([dict(P=x, Q=dy, out=dw)], GEMM_P_XC | GEMM_Q_XC | GEMM_OUT_F32, EPI_NONE, tile)
    return dw


_ColsumDesc = _cabi.STRUCTS["bq_colsum_desc"]


def _colsum_grouped_into(mats, outs, site):
    """outs[p] += the column sums of mats[p] (bf16 (M_p, N_p), fp32 (N_p,) contiguous) in the fixed-order form of the
    deterministic mode: partials per 512-row block, folded in row-block order by a second launch"""
    n = len(mats)
    arr = (_ColsumDesc * n)()
    for k, (m, o) in enumerate(zip(mats, outs)):
        _mat(m, "g")
        if m.dtype != torch.bfloat16 or o.dtype != torch.float32 or not o.is_contiguous() or o.numel() != m.shape[1]:
            raise RuntimeError("colsum_grouped: bf16 (M, N) matrices into contiguous fp32 (N,) sums")
        arr[k].g, arr[k].out, arr[k].M, arr[k].N, arr[k].ld = m.data_ptr(), o.data_ptr(), m.shape[0], m.shape[1], m.stride(0)
    dev = mats[0].device
    with torch.cuda.device(dev):
        part = torch.empty(max(1, _lib.bq_colsum_grouped_det_floats(arr, n)), dtype=torch.float32, device=dev)
        _check(_det_entry(site)(arr, n, _p(part), _stream()), "colsum_grouped_det")


def colsum_grouped(mats):
    """fp32 column sums of several bf16 (M_p, N_p) matrices (contiguous last dim) in one launch; returns a list of
    (N_p,) views of ONE zero-initialised buffer (one memset + one kernel for all bias gradients of a backward pass;
    in the deterministic mode a fixed-order fold as a second launch instead of float atomics)"""
    n = len(mats)
    dev = mats[0].device
    if _det():
        with torch.cuda.device(dev):
            flat = torch.zeros(sum(m.shape[1] for m in mats), dtype=torch.float32, device=dev)
        outs, off = [], 0
        for m in mats:
            outs.append(flat[off:off + m.shape[1]])
            off += m.shape[1]
        _colsum_grouped_into(mats, outs, "colsum_grouped")
        return outs
    with torch.cuda.device(dev):
        flat = torch.zeros(sum(m.shape[1] for m in mats), dtype=torch.float32, device=dev)
        arr = (_ColsumDesc * n)()
        outs, off = [], 0
        for k, m in enumerate(mats):
            _mat(m, "g")
            if m.dtype != torch.bfloat16:
                raise RuntimeError("colsum_grouped: bf16 only")
            o = flat[off:off + m.shape[1]]
            off += m.shape[1]
            outs.append(o)
            arr[k].g, arr[k].out, arr[k].M, arr[k].N, arr[k].ld = m.data_ptr(), o.data_ptr(), m.shape[0], m.shape[1], m.stride(0)
        _check(_lib.bq_colsum_grouped_bf16(arr, n, _stream()), "colsum_grouped")
    return outs


def wgrad_rows_ok(Ni, Nj):
    return bool(_lib.bq_wgrad_rows_supported(int(Ni), int(Nj)))


def wgrad_rows(x, dy, out, workgroups=0):
    """out (Nj, ldo) fp32 = dy^T x over whole rows: x (R, Ni) bf16 rows of stride ldp, dy (R, Nj) bf16; every operand row
    read once, per-workgroup partial products summed by a second kernel (bq_wgrad_rows_bf16; the detector's SharedMLP
    weight gradients).  out must be a whole (Nj, ldo) buffer: its columns [Ni, ldo) are zeroed."""
    _mat(x, "x"), _mat(dy, "dy")
    if out.dtype != torch.float32 or out.stride(1) != 1 or x.shape[0] != dy.shape[0] or out.shape[0] != dy.shape[1]:
        raise RuntimeError("wgrad_rows: out must be fp32 (Nj, ldo) rows, x and dy the same number of rows")
    with torch.cuda.device(x.device):
        w = _lib.bq_wgrad_rows_workgroups(x.shape[0], x.shape[1], dy.shape[1], int(workgroups))
        part = torch.empty(w * dy.shape[1] * out.stride(0), dtype=torch.float32, device=x.device)
        _check(_lib.bq_wgrad_rows_bf16(_p(x), _p(dy), _p(out), _p(part), x.shape[0], x.shape[1], dy.shape[1], x.stride(0),
                                       dy.stride(0), out.stride(0), int(workgroups), _stream()), "wgrad_rows")
    return out


# ---- SharedMLP layer on point-major rows: 1x1 convolution + BatchNorm statistics in its epilogue (csrc/gemm.hip) ----


def pwconv_bn_relu_fwd(x, K, w_pad, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, S, relu,
                       pool, center=None, want_arg=False, x_stats=None, defer_apply=False):
    """x: bf16 rows (R, ldx) view with contiguous elements (ldx = x.stride(0) >= K, the first K of a row are the input
    channels); w_pad: bf16 (N, Kc) contiguous, zero beyond K, Kc % 64 == 0.  y_raw = x @ w^T (bf16 (R, N)), its
    training-mode BatchNorm statistics from the fp32 accumulators (running buffers updated in place), then
    out = relu?(bn(y_raw)) as bf16 (R, N), or (R // S, N) = max over every run of S rows when pool.
    center (f32 (N,), e.g. running_mean itself): y_raw holds x @ w^T - center and stats describe the stored values (same
    `out`; the bf16 rounding of y_raw then applies to the deviation from the channel mean -- bq_pwconv_bn_fwd).
    Returns out, y_raw, stats (f32 (4, N): scale, shift, mean, rstd); with want_arg (pooled layers) a fourth value: u8
    (R // S, N), the row of each group's first maximum (None where the fp32-accumulator apply pass produced the output).
    Deferred activations between the layers of a SharedMLP (bq_pwconv_bn_fwd_x): x_stats = the previous layer's stats when x
    is that layer's y_raw (the input is then relu(x * x_stats[0] + x_stats[1]), applied tile by tile inside the kernel);
    defer_apply: skip this layer's own BatchNorm + ReLU pass -- out is None and the next layer reads y_raw."""
    if not x.is_cuda:
        raise RuntimeError("x: CPU not supported")
    R, N, Kc = x.shape[0], w_pad.shape[0], w_pad.shape[1]
    arg = None
    with torch.cuda.device(x.device):
        y_raw = torch.empty(R, N, dtype=torch.bfloat16, device=x.device)
        stats = torch.empty(5, N, dtype=torch.float32, device=x.device)   # scale, shift, mean, rstd (of the stored y) | shift_acc
        part = torch.empty(_lib.bq_pwconv_records(R, N) * 3 * N, dtype=torch.float32, device=x.device)
        _check(_lib.bq_pwconv_bn_fwd_x(_p(x), _p(x_stats[0]) if x_stats is not None else None,
                                       _p(x_stats[1]) if x_stats is not None else None, R, int(K), x.stride(0), _p(w_pad),
                                       w_pad.stride(0), Kc, N, _p(y_raw), _p(part), _p(gamma), _p(beta), _p(running_mean),
                                       _p(running_var), _p(num_batches_tracked), float(eps), float(momentum), _p(stats[0]),
                                       _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(center), _p(stats[4]), _stream()),
               "pwconv_bn_fwd")
        if defer_apply:
            return (None, y_raw, stats, None) if want_arg else (None, y_raw, stats)
        out = torch.empty(R // S if pool else R, N, dtype=torch.bfloat16, device=x.device)
        if FP32_PREACT[0] and (not pool or (int(S) in (16, 32, 64) and R % int(S) == 0)):
            # BatchNorm + ReLU (+ max-pool) on the fp32 accumulators of the product computed once more: the output never
            # passes through the bf16 y_raw (which the backward still reads)
            _check(_lib.bq_pwconv_bn_apply(_p(x), R, int(K), x.stride(0), _p(w_pad), w_pad.stride(0), Kc, N, _p(stats[0]),
                                           _p(stats[4]), _p(out), int(S), int(bool(relu)), int(bool(pool)),
                                           _stream()), "pwconv_bn_apply")
        else:
            if want_arg and pool and int(S) <= 256:
                arg = torch.empty(R // S, N, dtype=torch.uint8, device=x.device)
            _check(_lib.bq_bn_apply_arg(_p(y_raw), _p(stats[0]), _p(stats[1]), _p(out), _p(arg), R, N, int(S),
                                        int(bool(relu)), int(bool(pool)), _stream()), "bn_apply")
    return (out, y_raw, stats, arg) if want_arg else (out, y_raw, stats)


# ---- the backward of a SharedMLP layer in one pass over its activations (csrc/detbwd.hip) ------------------------------------
# a layer's fused backward can also sum the PREVIOUS layer's dbeta / dgamma (its dOut and its pre-activation are both in the pass:
# "the BatchNorm reduce in the epilogue of the next layer's dX GEMM").  Built, parity-green, and SLOWER: the second barrier per
# tile, the table reads and 32 more live registers per lane cost the fused kernels more than the eight reduction launches they
# replace (c2 7.72 / 7.77 -> 7.91 / 7.95 ms, c3 33.50 -> 33.41 inside the noise).  Off; BQ_CARRY_REDUCE=1 switches it on.
CARRY_REDUCE = [os.environ.get("BQ_CARRY_REDUCE", "0") == "1"]
# SharedMLP layers hand their stored pre-activation to the next layer, which applies BatchNorm + ReLU on load (no bn_apply pass,
# no activation tensor between two convolutions); off / BQ_DEFER_BN=0: every layer writes its activation
DEFER_BN = [os.environ.get("BQ_DEFER_BN", "1") != "0"]
# SharedMLP backward as reduction + one fused pass (off, or BQ_FUSED_SA_BWD=0 for A/B runs: bn_relu_bwd + dX GEMM + wgrad_rows)
FUSED_SA_BWD = [os.environ.get("BQ_FUSED_SA_BWD", "1") != "0"]


def bn_apply(y_raw, stats, S, relu, pool):
    """relu?(y_raw * stats[0] + stats[1]) as bf16 (R, N), or the max over runs of S rows (R // S, N) when pool"""
    R, N = y_raw.shape
    with torch.cuda.device(y_raw.device):
        out = torch.empty(R // S if pool else R, N, dtype=torch.bfloat16, device=y_raw.device)
        _check(_lib.bq_bn_apply(_p(y_raw), _p(stats[0]), _p(stats[1]), _p(out), R, N, int(S), int(bool(relu)),
                                int(bool(pool)), _stream()), "bn_apply")
    return out


def sa_bwd_supported(ldx, N, S, pool, need_dx):
    return bool(_lib.bq_sa_bwd_supported(int(ldx), int(N), int(S), int(bool(pool)), int(bool(need_dx))))


def bn_bwd_reduce(dy, x, stats, S, relu, pool, arg=None):
    """dgb f32 (2, C) = dbeta | dgamma of bn_relu_bwd alone; arg (pooled layers): the forward's arg-max table"""
    R, C = x.shape
    with torch.cuda.device(x.device):
        dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
        part = torch.empty(_lib.bq_bn_chunks(R, int(S), int(bool(pool))) * 2 * C, dtype=torch.float32, device=x.device)
        if pool and arg is not None and C <= 256 and 256 % C == 0:
            _check(_lib.bq_bn_backward_reduce_arg(_p(dy), _p(x), _p(arg), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]),
                                                  _p(part), _p(dgb), R, C, int(S), int(bool(relu)), _stream()),
                   "bn_backward_reduce_arg")
        else:
            _check(_lib.bq_bn_backward_reduce(_p(dy), _p(x), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(part),
                                              _p(dgb), R, C, int(S), int(bool(relu)), int(bool(pool)), _stream()),
                   "bn_backward_reduce")
    return dgb


def sa_bwd_fused(x, y_raw, dout, arg, w_pad, stats, dgb, S, relu, pool, need_dx, x_stats=None, carry_reduce=False):
    """x bf16 (R, ldx) whole padded rows, y_raw bf16 (R, N), dout bf16 (R, N) | (R // S, N) with arg u8 when pool, w_pad bf16
    (N, Kc), stats f32 (>= 4, N), dgb f32 (2, N) -> dx bf16 (R, ldx) | None, dw f32 (N, ldx).  x_stats: x is the previous
    layer's stored pre-activation and the layer's input relu(x * x_stats[0] + x_stats[1]) (bq_sa_bwd_fused_x; dx required);
    carry_reduce (with x_stats): a third value, f32 (2, ldx) = the PREVIOUS layer's dbeta | dgamma summed in the same pass
    (bq_sa_bwd_fused_xr), or None where the shape has no room for it"""
    R, ldx = x.shape[0], x.stride(0)
    N = y_raw.shape[1]
    with torch.cuda.device(x.device):
        dx = torch.empty(R, ldx, dtype=torch.bfloat16, device=x.device) if need_dx else None
        dw = torch.empty(N, ldx, dtype=torch.float32, device=x.device)
        wgs = _lib.bq_sa_bwd_workgroups(R, ldx, N, int(bool(pool)), int(bool(need_dx)))
        part = torch.empty(wgs * N * ldx, dtype=torch.float32, device=x.device)
        carry = bool(carry_reduce and x_stats is not None and need_dx
                     and _lib.bq_sa_bwd_reduce_supported(ldx, N, int(S), int(bool(pool))))
        red_part = torch.empty(wgs * 4 * 2 * ldx, dtype=torch.float32, device=x.device) if carry else None
        red_dgb = torch.empty(2, ldx, dtype=torch.float32, device=x.device) if carry else None
        xs = x_stats
        _check(_lib.bq_sa_bwd_fused_xr(_p(x), _p(xs[0]) if xs is not None else None, _p(xs[1]) if xs is not None else None,
                                       _p(xs[2]) if carry else None, _p(xs[3]) if carry else None, _p(red_part), _p(red_dgb),
                                       _p(y_raw), _p(dout), _p(arg), _p(w_pad), _p(stats[0]), _p(stats[1]), _p(stats[2]),
                                       _p(stats[3]), _p(dgb), _p(dx), _p(dw), _p(part), R, ldx, N, w_pad.stride(0), ldx, int(S),
                                       int(bool(relu)), int(bool(pool)), _stream()), "sa_bwd_fused")
    return (dx, dw, red_dgb) if carry_reduce else (dx, dw)


# SharedMLP outputs from the fp32 accumulators (bq_pwconv_bn_apply) instead of from the stored bf16 y.  OFF: measured in round 5
#  -- the layer output's error drops to one bf16 rounding, the 200-step convergence gap to fp32 does NOT
# close (+7.2 % against +3.3 % with the stored pre-activation, fp32's own spread 13 %) and the c3 step costs 1.3 ms more
FP32_PREACT = [False]


# ---- LM head + label-smoothed cross entropy (csrc/lmhead.hip + the cross-entropy epilogue of csrc/gemm.hip) -----------


def lmhead_ce_fwd(h, w, bias_pad, target, V, label_smoothing):
    """h bf16 (R, D), w bf16 (V, D) (contiguous), bias_pad f32 (Vp,) with Vp = V rounded up to 64 and zeros beyond V,
    target int32 (R,) (< 0: ignored).  Returns logits bf16 (R, Vp) (columns >= V are padding), loss f32 (R,), lse f32 (R,)."""
    R, D = h.shape
    Vp = bias_pad.numel()
    tiles_i = (Vp + 255) // 256
    with torch.cuda.device(h.device):
        logits = torch.empty(R, Vp, dtype=torch.bfloat16, device=h.device)
        part = torch.empty(tiles_i * 2, R, 3, dtype=torch.float32, device=h.device)
        zt = torch.zeros(R, dtype=torch.float32, device=h.device)
        loss = torch.empty(R, dtype=torch.float32, device=h.device)
        lse = torch.empty(R, dtype=torch.float32, device=h.device)
        # P = the vocabulary matrix with its TRUE extent in p_bytes (rows V .. Vp-1 of the last tile are out of bounds
        # for the bounds-checked LDS-DMA: zeros), Ni = the padded width of the logits
        gemm_grouped([dict(P=w, Q=h, out=logits, bias=bias_pad, out2=part, aux=target, colsum=zt, ksplit=V, Ni=Vp,
                           p_bytes=w.shape[0] * w.stride(0) * 2)], 0, EPI_BIAS_CE, 256)
        _check(_lib.bq_lmhead_ce_combine(_p(part), _p(zt), _p(target), _p(loss), _p(lse), R, tiles_i * 2, int(V),
                                         float(label_smoothing), _stream()), "lmhead_ce_combine")
    return logits, loss, lse


def lmhead_ce_dlogits(logits, lse, target, grad_loss, V, label_smoothing):
    """logits (R, Vp) bf16 from lmhead_ce_fwd -> dlogits IN PLACE (returned)"""
    R, Vp = logits.shape
    with torch.cuda.device(logits.device):
        _check(_lib.bq_lmhead_ce_dlogits(_p(logits), _p(lse), _p(target), _p(grad_loss), R, int(V), logits.stride(0),
                                         float(label_smoothing), _stream()), "lmhead_ce_dlogits")
    return logits


# ---- detection loss + gradient in two launches (csrc/detloss.hip) ---------------------------------------------------------
_DET_SCORES = ("objectness_scores", "heading_scores", "heading_residuals_normalized", "size_scores",
               "size_residuals_normalized", "sem_cls_scores")
_DET_TERM = {"vote_xyz": 0, "objectness_scores": 1, "center": 2, "heading_scores": 3, "heading_residuals_normalized": 4,
             "size_scores": 5, "size_residuals_normalized": 6, "sem_cls_scores": 7}


_DetLossDesc = _cabi.STRUCTS["bq_det_loss_desc"]
_DetLossSeg = _cabi.STRUCTS["bq_det_loss_seg"]


def det_score_ld(v, K):
    """row stride (floats per proposal) of a score tensor (B, K, w) or (B, K, NS, 3) the kernel can read in place: unit stride
    inside a row, rows `ld` apart, batches K * ld apart (a contiguous tensor, or a channel slice of the head output); else None"""
    w = v.shape[2] * (v.shape[3] if v.dim() == 4 else 1)
    ld = v.stride(1)
    if v.stride(-1) != 1 or ld < w or v.stride(0) != K * ld or (v.dim() == 4 and v.stride(2) != v.shape[3]):
        return None
    return ld


def det_loss_packing(t):
    """The six score tensors of the proposal head are slices of ONE (B, K, channels) tensor (proposal_module.decode_scores):
    -> (base, {name: (channel offset, width)}, channels) when they all are views, INSIDE the autograd graph, of the same
    contiguous base with one row stride -- the gradient is then produced for the base in one buffer; else None (the tensors
    are differentiated one by one, e.g. graphed.wrap_loss' fresh leaves)"""
    base = getattr(t[_DET_SCORES[0]], "_base", None)
    if base is None or not base.is_contiguous() or base.dtype != torch.float32 or not base.requires_grad:
        return None
    B, K = t["center"].shape[:2]
    if base.numel() % (B * K):
        return None
    ld = base.numel() // (B * K)
    off = {}
    for n in _DET_SCORES:
        v = t[n]
        if getattr(v, "_base", None) is not base or v.grad_fn is None or det_score_ld(v, K) != ld:
            return None
        o = v.storage_offset() - base.storage_offset()
        width = v.shape[2] * (v.shape[3] if v.dim() == 4 else 1)
        if o < 0 or o + width > ld:
            return None
        off[n] = (o, width)
    return base, off, ld


def det_loss_fwd(t, mean_size, near, far, w_neg, w_pos, packing=None):
    """t: dict of the tensors named in bq_det_loss_desc (fp32 outputs / labels, int64 class labels and masks; seed_inds int32
    or int64).  packing: det_loss_packing(t) -- the score tensors as slices of one head output: their gradients then land in
    ONE buffer shaped like it.  -> terms f32 (16,), objectness_label i64 (B,K), objectness_mask f32 (B,K), object_assignment
    i64 (B,K), grads {name or "packed": tensor}"""
    dev = t["center"].device
    B, K = t["center"].shape[:2]
    S = t["seed_xyz"].shape[1]
    VF = t["vote_xyz"].shape[1] // S
    N, G = t["vote_label"].shape[1], t["center_label"].shape[1]
    NH, NS, NC = t["heading_scores"].shape[2], t["size_scores"].shape[2], t["sem_cls_scores"].shape[2]
    d = _DetLossDesc()
    plain = ["seed_xyz", "vote_xyz", "aggregated_vote_xyz", "center", "vote_label", "center_label", "box_label_mask",
             "heading_residual_label", "size_residual_label"]
    for n in plain:
        _req(t[n], torch.float32, n)
        setattr(d, n, _p(t[n]))
    for n in ("vote_label_mask", "heading_class_label", "size_class_label", "sem_cls_label"):
        if t[n].dtype != torch.int64 or not t[n].is_contiguous() or not t[n].is_cuda:
            raise RuntimeError("%s must be a contiguous int64 device tensor" % n)
        setattr(d, n, _p(t[n]))
    si = t["seed_inds"]
    if si.dtype not in (torch.int32, torch.int64) or not si.is_contiguous():
        raise RuntimeError("seed_inds must be a contiguous int32 / int64 tensor")
    d.seed_inds, d.seed_inds_i64 = _p(si), int(si.dtype == torch.int64)
    _req(mean_size, torch.float32, "mean_size_arr")
    d.mean_size_arr = _p(mean_size)
    with torch.cuda.device(dev):
        terms = torch.zeros(16, dtype=torch.float32, device=dev)
        lab = torch.empty(B, K, dtype=torch.int64, device=dev)
        msk = torch.empty(B, K, dtype=torch.float32, device=dev)
        asg = torch.empty(B, K, dtype=torch.int64, device=dev)
        scratch = torch.empty(B * G + 1024, dtype=torch.int32, device=dev)
        grads = {"vote_xyz": torch.empty_like(t["vote_xyz"]), "center": torch.empty_like(t["center"])}
        d.g_vote_xyz, d.g_center = _p(grads["vote_xyz"]), _p(grads["center"])
        if packing:
            base, off, ld = packing
            gp = grads["packed"] = torch.empty_like(base)
            for n in _DET_SCORES:
                setattr(d, n, t[n].data_ptr())
                setattr(d, "g_" + n, gp.data_ptr() + 4 * off[n][0])
                setattr(d, "ld_" + n, ld)
        else:
            for n in _DET_SCORES:
                v = t[n]
                ld = det_score_ld(v, K)
                if ld is None or v.dtype != torch.float32 or not v.is_cuda:
                    raise RuntimeError("%s: fp32 device rows with unit stride expected" % n)
                grads[n] = torch.empty_strided(v.shape, v.stride(), dtype=torch.float32, device=dev)   # (same row stride)
                setattr(d, n, v.data_ptr())
                setattr(d, "g_" + n, grads[n].data_ptr())
                setattr(d, "ld_" + n, ld)
        d.terms, d.objectness_label, d.objectness_mask, d.object_assignment, d.scratch = _p(terms), _p(lab), _p(msk), _p(asg), _p(scratch)
        d.B, d.S, d.VF, d.N, d.K, d.G, d.NH, d.NS, d.NC = B, S, VF, N, K, G, NH, NS, NC
        d.cl_ld = t["center_label"].shape[2]
        d.near_threshold, d.far_threshold, d.objectness_weight_neg, d.objectness_weight_pos = near, far, w_neg, w_pos
        _check(_lib.bq_det_loss_fwd(ctypes.byref(d), _stream()), "det_loss_fwd")
    return terms, lab, msk, asg, grads


def det_loss_bwd(grads, upstream, packing=None):
    """grads: det_loss_fwd's buffers, upstream f32 (8,) -> {name or "packed": g * upstream[term]}, ONE launch"""
    outs = {k: torch.empty_strided(g.shape, g.stride(), dtype=g.dtype, device=g.device) for k, g in grads.items()}
    segs = []

    def seg(g, o, g_off, rows, width, ld, term):
        segs.append(_DetLossSeg(g.data_ptr() + 4 * g_off, o.data_ptr() + 4 * g_off, rows, width, ld, term))
    for n in ("vote_xyz", "center"):
        seg(grads[n], outs[n], 0, grads[n].numel() // 3, 3, 3, _DET_TERM[n])
    if packing:
        base, off, ld = packing
        rows = base.numel() // ld
        covered = sorted((o, w, n) for n, (o, w) in off.items())
        pos = 0
        for o, w, n in covered:
            if o > pos:
                seg(grads["packed"], outs["packed"], pos, rows, o - pos, ld, -1)   # channels no term reads (the centre offsets)
            seg(grads["packed"], outs["packed"], o, rows, w, ld, _DET_TERM[n])
            pos = o + w
        if pos < ld:
            seg(grads["packed"], outs["packed"], pos, rows, ld - pos, ld, -1)
    else:
        for n in _DET_SCORES:
            g = grads[n]
            w = g.shape[2] * (g.shape[3] if g.dim() == 4 else 1)
            seg(g, outs[n], 0, g.shape[0] * g.shape[1], w, g.stride(1), _DET_TERM[n])
    arr = (_DetLossSeg * len(segs))(*segs)
    with torch.cuda.device(upstream.device):
        _check(_lib.bq_det_loss_bwd(arr, len(segs), _p(upstream), _stream()), "det_loss_bwd")
    return outs


# ---- deterministic scatter gradients through an inverted index (csrc/invert.hip) ---------------------------------------------
DETERMINISTIC_SCATTER = [True]


def invert_index(idx, N):
    """idx int32 (B, ...) with values in [0, N) -> (start int32 (B * N + 1,), slots int32-sized uint32 (B * L,)): for scene b
    and value v the positions b * L + l with idx[b].flatten()[l] == v are slots[start[b * N + v] : start[b * N + v + 1]],
    ascending"""
    _req(idx, torch.int32, "idx")
    B = idx.shape[0]
    L = idx.numel() // max(B, 1)
    with torch.cuda.device(idx.device):
        start = torch.empty(B * int(N) + 1, dtype=torch.int32, device=idx.device)
        slots = torch.empty(max(B * L, 1), dtype=torch.int32, device=idx.device)
        nbytes = int(_lib.bq_invert_index_workspace_bytes(B * L))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=idx.device)
        _check(_lib.bq_invert_index(_p(idx), B, L, int(N), _p(start), _p(slots), _p(ws), nbytes, _stream()), "invert_index")
    return start, slots


def group_concat_pm_grad_gather(grad_out, inv, n, radius=1.0, normalize=False, need_features=True, need_xyz=False,
                                need_new_xyz=False):
    """the gradients of group_concat_pm as gathers over inv = invert_index(idx, n): grad_out (B, M, S, 3 + C) rows (contiguous
    or padded rows of a uniform stride % 8 == 0) -> (grad_feats f32 (B, n, C) | None, grad_xyz f32 (B, n, 3) | None,
    grad_new_xyz f32 (B, M, 3) | None); None (a single value) when the layout is not the kernel's"""
    B, M, S, CT = grad_out.shape
    C = CT - 3
    ld = grad_out.stride(2)
    if (grad_out.stride(3) != 1 or grad_out.stride(1) != S * ld or grad_out.stride(0) != M * S * ld or ld < CT or ld % 8
            or grad_out.data_ptr() % 16 or grad_out.dtype not in (torch.bfloat16, torch.float32)):
        return None
    need_features = bool(need_features) and C > 0
    if not (need_features or need_xyz or need_new_xyz):
        return None, None, None
    dev = grad_out.device
    with torch.cuda.device(dev):
        gf = torch.empty(B, int(n), C, dtype=torch.float32, device=dev) if need_features else None
        gx = torch.empty(B, int(n), 3, dtype=torch.float32, device=dev) if need_xyz else None
        gn = torch.empty(B, M, 3, dtype=torch.float32, device=dev) if need_new_xyz else None
        _check(_lib.bq_group_concat_pm_grad_gather(_p(grad_out), int(grad_out.dtype == torch.bfloat16), _p(inv[0]), _p(inv[1]),
                                                   _p(gf), _p(gx), _p(gn), B, C, int(n), M, S, ld, float(radius),
                                                   int(bool(normalize)), _stream()), "group_concat_pm_grad_gather")
    return gf, gx, gn


def three_interpolate_grad_gather(grad_out, inv, weight, m):
    """grad_out f32 (B, C, n) contiguous, inv = invert_index(idx (B, n, 3), m), weight f32 (B, n, 3) -> f32 (B, C, m)"""
    _req(grad_out, torch.float32, "grad_out"); _req(weight, torch.float32, "weight")
    B, C, n = grad_out.shape
    with torch.cuda.device(grad_out.device):
        out = torch.empty(B, C, int(m), dtype=torch.float32, device=grad_out.device)
        _check(_lib.bq_three_interpolate_grad_gather(_p(grad_out), _p(inv[0]), _p(inv[1]), _p(weight), _p(out), B, C, n, int(m),
                                                     _stream()), "three_interpolate_grad_gather")
    return out


# ---- eval-mode SharedMLP of one detector module in one launch (csrc/mlp_eval.hip) ----------------------------------------
_MlpEvalLayer = _cabi.STRUCTS["bq_mlp_eval_layer"]
_MlpEvalDesc = _cabi.STRUCTS["bq_mlp_eval_desc"]


MLP_EVAL_KMAX = 512     # input channels (rounded up to 32) the kernel stages
MLP_EVAL_S = (16, 32, 64)


def mlp_eval_width_ok(n):
    """a BatchNorm layer width the fused eval kernel covers"""
    return n % 32 == 0 and 32 <= n <= 256


def _mlp_eval_layer(dst, spec):
    """spec: dict(w=(n, ldw) bf16 rows, zero beyond the input width; mean, var, eps; optional gamma, beta, bias; relu)"""
    w = spec["w"]
    if w.dtype != torch.bfloat16 or w.dim() != 2 or w.stride(1) != 1:
        raise RuntimeError("mlp_eval: weights must be bf16 (n, ldw) rows")
    for k in ("gamma", "beta", "mean", "var", "bias"):
        t = spec.get(k)
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != w.device):
            raise RuntimeError("mlp_eval: %s must be a contiguous float tensor on the weights' device" % k)
    dst.w, dst.n, dst.ldw = w.data_ptr(), w.shape[0], w.stride(0)
    for k in ("gamma", "beta", "mean", "var", "bias"):
        setattr(dst, k, _p(spec.get(k)))
    dst.eps, dst.relu = float(spec.get("eps", 0.0)), int(bool(spec.get("relu", True)))


def mlp_eval(layers, tail=None, grouped=None, rows=None, pool=False):
    """One eval-mode detector module in one launch.  grouped = (xyz, new_xyz, feats_pm | None, idx, radius, normalize) -- the
    operands of group_concat_pm -- or rows = (x (R, >= K) bf16 rows with contiguous channels, K).  layers: 1..3 BatchNorm
    layer specs (see _mlp_eval_layer), tail: a last linear spec (w, bias) with fp32 output.  Returns bf16 (B M, n) maxima
    (pool), fp32 (R, n_tail) (tail) or bf16 (R, n) rows."""
    d = _MlpEvalDesc()
    if grouped is not None:
        xyz, new_xyz, feats, idx, radius, normalize = grouped
        _req(xyz, torch.float32, "xyz"); _req(new_xyz, torch.float32, "new_xyz"); _req(idx, torch.int32, "idx")
        B, N, _ = xyz.shape
        _, M, S = idx.shape
        d.xyz, d.new_xyz, d.idx = xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr()
        d.B, d.N, d.M, d.S, d.radius, d.normalize = B, N, M, S, float(radius), int(bool(normalize))
        if feats is not None:
            if not feats.is_cuda or feats.dtype != torch.float32 or feats.stride(2) != 1:
                raise RuntimeError("feats_pm must be a CUDA float tensor (B,N,C) with contiguous rows")
            d.feats, d.C, d.f_bs, d.f_rs = feats.data_ptr(), feats.shape[2], feats.stride(0), feats.stride(1)
        d.R = B * M * S
        dev, R = xyz.device, B * M * S
    else:
        x, K = rows
        if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
            raise RuntimeError("mlp_eval: rows must be a CUDA bf16 (R, ld) tensor with contiguous channels")
        d.x, d.ldx, d.K, d.R = x.data_ptr(), x.stride(0), int(K), x.shape[0]
        dev, R = x.device, x.shape[0]
    d.n_layers = len(layers)
    if not 1 <= len(layers) <= 3:
        raise RuntimeError("mlp_eval: %d layers (1..3)" % len(layers))
    for i, spec in enumerate(layers):
        _mlp_eval_layer(d.layers[i], spec)
    n = layers[-1]["w"].shape[0]
    with torch.cuda.device(dev):
        if tail is not None:
            d.has_tail = 1
            _mlp_eval_layer(d.tail, dict(tail, relu=False))
            out = torch.empty(R, tail["w"].shape[0], dtype=torch.float32, device=dev)
        elif pool:
            out = torch.empty(R // d.S, n, dtype=torch.bfloat16, device=dev)
        else:
            out = torch.empty(R, n, dtype=torch.bfloat16, device=dev)
        if R == 0:   # nothing to launch (and an empty tensor has no address to pass)
            return out
        d.out, d.pool = out.data_ptr(), int(bool(pool))
        _check(_lib.bq_mlp_eval(ctypes.byref(d), _stream()), "mlp_eval")
    return out
