"""Reference, bound, inputs and route table of the MFMA bf16 GEMM family (csrc/gemm.hip, csrc/gemm_mid.hip,
csrc/gemm64_kernel_body.h; bq_gemm_bf16 / _ext.gemm_grouped, bq_wgrad_rows_bf16) for tests/test_gemm_bound_cpu.py and
tests/test_gemm_bound_gpu.py.  Nothing here needs a GPU or the extension.

A problem is out[j][i] = epilogue(sum_k P[i][k] Q[j][k]); here P is always the LOGICAL (Ni, Kc) matrix and Q the logical
(Nj, Kc) one, whatever their storage (K-contiguous or contraction-major).

EXACT TIER.  Operands are bf16 tensors of small integers (P uniform in {-2..2}, Q in {-1, 0, 1}, bias in {-3..3}, aux in
{-4..4}).  Every product and every partial sum is then an integer below 2^24 -- conditions(): Kc max|P| max|Q| + max|bias| +
max|aux| < 2^24, an upper bound of sum_k |p||q| + |bias| + |aux| of every output -- so fp32 accumulation is exact in any order,
on any MFMA shape, across split-K atomics, stream-K slabs and the deterministic fold, and the kernel's answer is determined
bit for bit: expected() = the integer product (fp64 matmul: exact below 2^53) plus integer bias / aux, converted ONCE to the
output type (exact for fp32, round-to-nearest-even for bf16), compared with == on values.  For bf16 outputs at least 99 % of
the outputs of a case have |exact| <= 256 (bf16 holds every integer up to 256), so a change by one unit survives the rounding
(measured on the CPU: P in {-2..2}, Q in {-1, 0, 1} gives max |out| 326 and 6e-5 of the outputs above 256 at
(2000, 768, K = 3072), none at K = 768); the rest are still held to RNE_bf16(exact).

BOUND TIER.  fp64 reference r from the bf16 operands the kernel saw, per-element tolerance.  u = 2^-24, A = (|P| |Q|^T)_ji:
    e_acc = 2 Kc u A                   fp32 accumulation in any order; the factor 2 covers an MFMA whose internal adds are not
                                       round-to-nearest
    fp32 out:  e_acc + u |r|
    bf16 out:  2^-8 (|r| + e_acc) + e_acc
2^-8: bf16 keeps 8 significant bits, so round-to-nearest errs by up to 2^-8 relative just above a power of two (a 16-wide
blocked fp32 emulation at (130, 768, 768) reaches |err| / bound 0.75 with 2^-8 and 1.51 with 2^-9).
Non-linear epilogues, constants from csrc/gemm_common.h (fit and scan: DESIGN.md section 4.4):
    BIAS_GELU  out2 = gelu(out) is taken at the STORED bf16 pre-activation: reference gelu_erf(kernel's own out), tolerance
               3.1e-5 + 2^-8 |gelu|   (max |gelu_fit - gelu_erf| = 3.1e-5; bf16 rounding of the result)
    DGELU      r = acc64 gelu_erf'(aux), e = |gelu_erf'(aux)| e_acc + G |acc64| with G = 1.2e-4 (|d gelu_fit - gelu_erf'|), plus
               2e-5 where |aux| < 2^-16 (the LDS table of the 256 x 256 kernel clamps its index there); then the bf16 line.
    column sums of a bf16 output: both epilogues (gemm64_kernel_body.h `cs[r] += ok ? v[r]` after `v[r] = (float)(__bf16)v[r]`,
               gemm256_kernel `(float)(__bf16)v[r]` / `vv[b][r]`) add the ROUNDED values, so the reference is the fp64 column
               sum of the kernel's own stored output and the bound is the fp32 sum of Nj terms alone: Nj u sum_j |x_ji|.
    column sums of the weight-gradient form (colsum[j] = sum_k Q[j][k], from all-ones MFMAs): Kc u sum_k |Q[j][k]| x 2.

ROUTES.  kernel_ids() parses profiler kernel names (demangled or mangled) to ids such as gemm64_kernel<32,0,0,1,0,4,3>;
routes() restates -- independently of the product, which this file must not import -- which kernels a gemm_grouped call must
reach: the Python choice of tile (bridgeqa_amd/gemm_route.py: pick_tile, GEMM_TILE_ROWS, TILE256_MIN_K, the row-map fallback,
mid_ok) and the C++ choice of variant (csrc/gemm_common.h gemm_form() and streamk_fits(), the launchers' long_k and
four-K-tile rules, the _det kernels) together.  Moving a threshold in gemm_route.py, or a form in gemm_form(), means editing
this file in the same commit; tests/test_gemm_bound_cpu.py compares both with it without a device.
"""
import math
import re
import zlib

import torch

U = 2.0 ** -24
B8 = 2.0 ** -8
GELU_ERR = 3.1e-5       # gemm_common.h: max |gelu - gelu_erf|
DGELU_ERR = 1.2e-4      # gemm_common.h: |d gelu - gelu_erf'|
TAB_CLAMP = 2.0 ** -16  # gemm_common.h: the table index is clamped to 2^-16 .. 8
TAB_CLAMP_ERR = 2e-5    # "below 2^-16 Phi and gelu' are 0.5 to 2e-5"

P_XC, Q_XC, OUT_F32, BACKGROUND = 1, 2, 4, 8
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_BIAS_CE, EPI_ADD = 0, 1, 2, 3, 4, 5
MAX_PROBLEMS = 36       # bq_gemm_max_problems(); the GPU battery asserts it


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def int_tensor(shape, lo, hi, *key):
    """bf16 tensor of integers uniform in lo..hi, seeded by its key"""
    g = torch.Generator().manual_seed(_seed("int", shape, lo, hi, key))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.bfloat16)


def real_tensor(shape, scale, *key, spike=False):
    """bf16 normal values; spike: row 1 x 24 and the last column x 16, so that |P| |Q|^T is far from uniform"""
    g = torch.Generator().manual_seed(_seed("real", shape, key))
    t = torch.randn(*shape, generator=g) * scale
    if spike and t.dim() == 2:
        t[min(1, t.shape[0] - 1)] *= 24.0
        t[:, -1] *= 16.0
    return t.to(torch.bfloat16)


def operands(Ni, Nj, Kc, exact, tag=0):
    """logical P (Ni, Kc), Q (Nj, Kc), bias (Ni,), aux (Nj, Ni): integers (exact tier) or reals (bound tier).  Seeded by the
    shape, not by the case, so that equal shapes share their operands (and the CPU suite its products)."""
    if exact:
        return (int_tensor((Ni, Kc), -2, 2, "P", tag), int_tensor((Nj, Kc), -1, 1, "Q", tag),
                int_tensor((Ni,), -3, 3, "b", tag).float(), int_tensor((Nj, Ni), -4, 4, "aux", tag))
    return (real_tensor((Ni, Kc), 0.1, "P", tag, spike=True), real_tensor((Nj, Kc), 1.0, "Q", tag, spike=True),
            real_tensor((Ni,), 1.0, "b", tag).float(), real_tensor((Nj, Ni), 1.5, "aux", tag))


def conditions(P, Q, bias=None, aux=None):
    """upper bound of sum_k |p||q| + |bias| + |aux| over all outputs: the exact tier needs it below 2^24"""
    s = P.shape[1] * float(P.abs().max()) * float(Q.abs().max())
    if bias is not None:
        s += float(bias.abs().max())
    if aux is not None:
        s += float(aux.abs().max())
    return s


# ---- references -------------------------------------------------------------------------------------------------------------
def acc64(P, Q):
    """(Nj, Ni) fp64 product of the logical operands"""
    return Q.double() @ P.double().t()


def rne_bf16(x64):
    """an integer-valued (|x| < 2^24) fp64 tensor converted once to bf16, as fp64 values"""
    return x64.float().to(torch.bfloat16).double()


def expected(P, Q, bias=None, aux=None, f32=False):
    """exact tier: the integer result converted once to the output type (fp64 values)"""
    r = acc64(P, Q)
    if bias is not None:
        r = r + bias.double()[None, :]
    if aux is not None:
        r = r + aux.double()
    return r if f32 else rne_bf16(r)


def mismatches(out, want):
    """exact tier comparison: == on values (-0 equals +0, NaN equals nothing); returns the indices that differ"""
    return (~(out.double() == want.double())).nonzero()


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu_erf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def bound(P, Q, bias=None, aux=None, epi=EPI_NONE, f32=False, Kc=None):
    """bound tier: (r, tol) of out, both (Nj, Ni) fp64.  Kc: the contraction length the kernel walks (default P's)"""
    Kc = P.shape[1] if Kc is None else Kc
    r = acc64(P, Q)
    e = 2.0 * Kc * U * (Q.double().abs() @ P.double().abs().t())
    if epi in (EPI_BIAS, EPI_BIAS_GELU) and bias is not None:
        r = r + bias.double()[None, :]
        e = e + U * r.abs()                       # the fp32 add of the bias
    elif epi == EPI_ADD:
        r = r + aux.double()
        e = e + U * r.abs()
    elif epi == EPI_DGELU:
        a = aux.double()
        d = dgelu_erf(a)
        g = DGELU_ERR + TAB_CLAMP_ERR * (a.abs() < TAB_CLAMP).double()
        e = d.abs() * e + g * r.abs()
        r = r * d
        e = e + U * r.abs()                       # the fp32 multiplication
    if f32:
        return r, e + U * r.abs()
    return r, B8 * (r.abs() + e) + e


def gelu_bound(out_stored):
    """(r, tol) of out2 = gelu(stored bf16 pre-activation)"""
    r = gelu_erf(out_stored.double())
    return r, GELU_ERR + B8 * r.abs()


def colsum_bound(out_stored):
    """(r, tol) of the column sums over j of a stored bf16 output (Nj, Ni): the kernels add the rounded values"""
    x = out_stored.double()
    return x.sum(0), x.shape[0] * U * x.abs().sum(0)


def qsum_bound(Q):
    """(r, tol) of colsum[j] = sum_k Q[j][k] of the weight-gradient form"""
    q = Q.double()
    return q.sum(1), 2.0 * Q.shape[1] * U * q.abs().sum(1)


# ---- the norms of tests/test_gemm_gpu.py::_check, restated (what the planted defects must still pass) ---------------------------
def old_norms_accept(out, ref, f32=False):
    out, ref = out.float(), ref.float()
    rel = ((out - ref).norm() / (ref.norm() + 1e-20)).item()
    mx = ((out - ref).abs().max() / (ref.abs().max() + 1e-20)).item()
    return bool(torch.isfinite(out).all()) and rel <= (1e-5 if f32 else 3e-3) and mx <= (1e-4 if f32 else 1e-2)


# ---- CPU emulation of the kernels' rounding points ------------------------------------------------------------------------------
def emulate(P, Q, bias=None, aux=None, epi=EPI_NONE, f32=False, block=16):
    """fp32 accumulation in `block`-wide k slices (one MFMA each), the epilogue in fp32, one bf16 rounding; the GELU fit of
    gemm_common.h evaluated in fp32.  Returns (out, out2 or None) as the kernel would store them."""
    Pf, Qf = P.float(), Q.float()
    acc = torch.zeros(Q.shape[0], P.shape[0], dtype=torch.float32)
    for k in range(0, P.shape[1], block):
        acc = acc + Qf[:, k:k + block] @ Pf[:, k:k + block].t()
    if epi in (EPI_BIAS, EPI_BIAS_GELU) and bias is not None:
        acc = acc + bias.float()[None, :]
    if epi == EPI_ADD:
        acc = acc + aux.float()
    if epi == EPI_DGELU:
        acc = acc * dgelu_fit(aux.float())
    if f32:
        return acc, None
    out = acc.to(torch.bfloat16)
    out2 = gelu_fit(out.float()).to(torch.bfloat16) if epi == EPI_BIAS_GELU else None
    return out, out2


_A1, _A3, _A5 = 1.59525515, 7.38511083e-2, -6.82350683e-4


def _cdf_fit(x):
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    z = xc * (x2 * (x2 * _A5 + _A3) + _A1)
    return xc, x2, torch.sigmoid(z)


def gelu_fit(x):
    """gelu_f of gemm_common.h in fp32"""
    return x * _cdf_fit(x.float())[2]


def dgelu_fit(x):
    """dgelu_f of gemm_common.h in fp32"""
    xc, x2, s = _cdf_fit(x.float())
    u_ = xc * (x2 * (x2 * 5.0 * _A5 + 3.0 * _A3) + _A1)
    return u_ * (s - s * s) + s


# ---- routes -----------------------------------------------------------------------------------------------------------------
_KNAME = re.compile(r"(gemm(?:64|128|256)_kernel(?:_det)?|splitk_fold_det_kernel|wgrad_rows_reduce_kernel|wgrad_rows_kernel)"
                    r"(?:<([^>]*)>|I((?:L[a-z]\d+E)+)E)?")


def kernel_ids(names):
    """canonical ids ('gemm64_kernel<32,0,0,1,0,4,3>', 'splitk_fold_det_kernel') of the GEMM kernels among profiler kernel
    names, demangled ('void bq::gemm64_kernel<32, false, false, 1, false, 4, 3>(bq::GemmArgs)') or not
    ('_ZN2bq13gemm64_kernelILi32ELb0ELb0ELi1ELb0ELi4ELi3EEEvNS_8GemmArgsE')"""
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


GEMM_TILE_ROWS = 1024
TILE256_MIN_K = 2304
LONG_K_TILES = 12       # launch_gemm: two K tiles per step from 12 K tiles ...
LONG_K_MAX_TILES = 2048  # ... in launches of at most 2048 tiles
K4_MAX_TILES = 512      # launch_variant: four K tiles per step (tile 32) in launches of at most 512 tiles


def pick_tile(Ni, Nj, q_xc):
    if Nj >= GEMM_TILE_ROWS and Ni >= 256:
        return 128
    if q_xc or Nj > 512:
        return 64
    return 32


def auto_tile(problems, flags, epilogue):
    """the tile class _gemm_grouped_launch picks for tile=None"""
    pxc, qxc, f32 = bool(flags & P_XC), bool(flags & Q_XC), bool(flags & OUT_F32)
    t, all_mid, any_map = 32, True, False
    for p in problems:
        mid_ok = (not qxc and not f32 and p["Kc"] >= 128 and not p.get("colsum")
                  and epilogue in (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_ADD))
        all_mid = all_mid and mid_ok
        any_map = any_map or bool(p.get("map"))
        t = max(t, pick_tile(p["Ni"], p["Nj"], qxc))
    if t == 128 and not all_mid:
        t = 256
    if t == 128 and not pxc and epilogue in (EPI_NONE, EPI_BIAS) and all(p["Kc"] >= TILE256_MIN_K for p in problems):
        t = 256
    if t == 256 and any_map and not (pxc and qxc and f32):
        t = 64
    return t


def _cdiv(a, b):
    return (a + b - 1) // b


def launch_tiles(problems, tile, f32):
    tj, ti = (256 if tile == 256 else tile), (256 if tile in (256, 128) else 64)
    n = 0
    for p in problems:
        ks = p.get("ksplit", 1)
        n += _cdiv(p["Ni"], ti) * _cdiv(p["Nj"], tj) * (ks if (f32 and tile != 256 and ks > 1) else 1)
    return n


def _streamk_fits(nkt, tiles, slots):
    units = tiles * nkt
    rounds = _cdiv(tiles, slots)
    return (nkt >= 24 and tiles >= slots // 2 and units // slots >= 16 and rounds * nkt * slots >= units * 115 // 100
            and 8 * tiles <= 65536)


def routes(problems, flags, epilogue, tile=None, cus=256, det=False, streamk=0):
    """the set of GEMM kernel ids gemm_grouped(problems, flags, epilogue, tile) must launch.  problems: dicts with Ni, Nj, Kc
    and optionally ksplit, colsum (bool), map (bool: a q_rpb / o_rpb row map).  det: set_deterministic(True); streamk: bit 0
    streamk_enable, bit 1 streamk256_enable (the workspace is registered for single-problem tile-128 launches)."""
    pxc, qxc, f32 = bool(flags & P_XC), bool(flags & Q_XC), bool(flags & OUT_F32)
    t = tile or auto_tile(problems, flags, epilogue)
    background = bool(flags & BACKGROUND) and t == 128
    b = lambda v: "1" if v else "0"
    ids = set()
    if det and any(p.get("ksplit", 1) > 1 for p in problems):
        ids.add("splitk_fold_det_kernel")
    for c0 in range(0, len(problems), MAX_PROBLEMS):
        chunk = problems[c0:c0 + MAX_PROBLEMS]
        total = launch_tiles(chunk, t, f32)
        if det and f32 and t in (64, 32):
            ids.add("gemm64_kernel_det<%d,%s,%s,%d>" % (t, b(pxc), b(qxc), epilogue))
            continue
        long_k = t != 256 and total <= LONG_K_MAX_TILES and all(p["Kc"] >= 64 * LONG_K_TILES for p in chunk)
        if t == 128:
            p0 = chunk[0]
            sk_shape = (len(chunk) == 1 and len(problems) == 1 and not pxc and not qxc and not f32 and not background and not det)
            nkt = _cdiv(p0["Kc"], 64)
            if (streamk & 2 and sk_shape and epilogue in (EPI_NONE, EPI_BIAS) and not p0.get("colsum") and not p0.get("map")
                    and _streamk_fits(nkt, _cdiv(p0["Ni"], 256) * _cdiv(p0["Nj"], 256), cus)):
                ids.add("gemm256_kernel<0,0,%d,0,1>" % epilogue)
            elif streamk & 1 and sk_shape and epilogue in (EPI_NONE, EPI_BIAS, EPI_ADD) and _streamk_fits(nkt, total, 2 * cus):
                ids.add("gemm128_kernel<0,0,%d,0,16,1>" % epilogue)
            else:
                ids.add("gemm128_kernel<%s,%s,%d,%s,16,0>" % (b(pxc), b(qxc), epilogue, b(f32)))
        elif t == 256:
            ids.add("gemm256_kernel<%s,%s,%d,%s,0>" % (b(pxc), b(qxc), epilogue, b(f32)))
        else:
            kt2_ok = not f32 and not qxc
            kt = 1
            if kt2_ok and long_k:
                kt = 4 if (t == 32 and total <= K4_MAX_TILES) else 2
            ids.add("gemm64_kernel<%d,%s,%s,%d,%s,%d,3>" % (t, b(pxc), b(qxc), epilogue, b(f32), kt))
    return ids


def wgrad_rows_routes(Ni, Nj):
    return {"wgrad_rows_kernel<%d,%d>" % (_cdiv(Ni, 64), _cdiv(Nj, 64)), "wgrad_rows_reduce_kernel"}


def wgrad_rows_supported(Ni, Nj):
    ti, tj = _cdiv(Ni, 64), _cdiv(Nj, 64)
    return 1 <= ti <= 5 and tj in (1, 2, 4) and ti + tj <= 7 and not (ti == 5 and tj == 1)


# ---- every instantiation launch_gemm, launch_gemm_mid and bq_wgrad_rows_bf16 can reach (csrc/gemm_common.h gemm_form()) ------------
def _route_table():
    t = []
    bf16_forms = [(0, (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_ADD)), (1, (EPI_NONE, EPI_DGELU, EPI_ADD))]
    for pxc, epis in bf16_forms:
        for e in epis:
            for bj, kts in ((64, (1, 2)), (32, (1, 2, 4))):
                t += ["gemm64_kernel<%d,%d,0,%d,0,%d,3>" % (bj, pxc, e, k) for k in kts]
            t.append("gemm128_kernel<%d,0,%d,0,16,0>" % (pxc, e))
            if pxc or e not in (EPI_DGELU, EPI_ADD):     # (tile 256 has no K-contiguous DGELU / ADD form)
                t.append("gemm256_kernel<%d,0,%d,0,0>" % (pxc, e))
    for bj in (64, 32):                                  # fp32 outputs of the small tiles, atomic and deterministic
        for pxc, e in ((0, EPI_NONE), (0, EPI_BIAS), (1, EPI_NONE)):
            t += ["gemm64_kernel<%d,%d,0,%d,1,1,3>" % (bj, pxc, e), "gemm64_kernel_det<%d,%d,0,%d>" % (bj, pxc, e)]
    t += ["gemm64_kernel<64,1,1,0,1,1,3>", "gemm64_kernel_det<64,1,1,0>", "gemm128_kernel<1,1,0,1,16,0>",
          "gemm256_kernel<1,1,0,1,0>", "splitk_fold_det_kernel"]
    t += ["gemm128_kernel<0,0,%d,0,16,1>" % e for e in (EPI_NONE, EPI_BIAS, EPI_ADD)]      # stream-K, 256 x 128
    t += ["gemm256_kernel<0,0,%d,0,1>" % e for e in (EPI_NONE, EPI_BIAS)]                  # stream-K, 256 x 256
    t += ["wgrad_rows_kernel<%d,%d>" % (i, j) for i in range(1, 6) for j in (1, 2, 4) if wgrad_rows_supported(64 * i, 64 * j)]
    t.append("wgrad_rows_reduce_kernel")
    return t


ROUTE_TABLE = _route_table()
# instantiations in the library that are out of this suite's scope (none is left that no permitted combination reaches)
NOT_REACHED = {
    "gemm256_kernel<0,0,4,0,0>": "EPI_BIAS_CE, the LM-head cross-entropy epilogue: not launched by this battery; held to its own bound by tests/test_lmhead_bound_gpu.py",
    "pwconv64_kernel / pwconv64s_kernel": "the SharedMLP convolution kernels: out of scope (tests/test_modules_gpu.py)",
}
