"""CPU checks of tests/gemm_ref.py, the reference the GPU battery of tests/test_gemm_bound_gpu.py holds the GEMM family to:

  * the exact tier's conditions on the battery's operand generators, for every problem shape the battery uses;
  * a CPU emulation of the kernels' rounding points (fp32 accumulation in 16- and 32-wide blocks, one bf16 rounding, the GELU
    fit in fp32) stays within the bound tier on every element -- |err| / bound <= 1 and no more: one correct bf16 rounding
    just above a power of two already uses nearly all of the 2^-8 term;
  * planted defects, each confined to ONE tile of an otherwise correct result, all fail the exact tier; L2_ACCEPTS /
    BOTH_ACCEPT record which of them the two numbers of tests/test_gemm_gpu.py::_check accept at the ViT shape, BOUND_BLIND
    which of them the bound tier cannot see at K = 3072 -- the reason the exact tier exists;
  * the kernel-name parser on both name forms; routes() at both sides of every threshold.
"""
import ast
import os

import pytest
import torch

import gemm_ref as R
from gemm_ref import EPI_ADD, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_NONE, OUT_F32, P_XC, Q_XC

DW = P_XC | Q_XC | OUT_F32


def _battery_shapes():
    """every dict(Ni=.., Nj=.., Kc=..) literal of the GPU battery, read from its source (importing it would need the marker
    machinery of a GPU run); loops over names are expanded by hand below"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gemm_bound_gpu.py")).read()
    shapes = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "dict":
            kw = {k.arg: k.value for k in node.keywords}
            if {"Ni", "Nj", "Kc"} <= set(kw) and all(isinstance(kw[n], ast.Constant) for n in ("Ni", "Nj", "Kc")):
                shapes.add((kw["Ni"].value, kw["Nj"].value, kw["Kc"].value))
    # the shapes the battery builds in loops: product shapes, ragged extents, K tails, thresholds
    M = 16400
    for N, K in ((768, 768), (2304, 768), (3072, 768), (768, 3072), (768, 2304)):
        shapes |= {(N, M, K), (N, K, M)} | {(N, m, K) for m in (80, 320, 640)}
    shapes |= {(Ni, Nj, 192) for Ni in (8, 72, 264) for Nj in (1, 7, 257, 1000, 16400)}
    shapes |= {(72, 257, K) for K in (64, 128, 832, 960)} | {(264, 3300, K) for K in (832, 960)}
    shapes |= {(264, 136, m) for m in (20, 63, 64, 65, 1000, 16400)}
    shapes |= {(64, 65537, 768), (768, 2000, 2304), (264, 600, 768)}
    return sorted(shapes)


def test_exactness_conditions_hold_for_every_battery_shape():
    """(1) every partial sum below 2^24 in any order; (2) at least 99 % of the bf16 outputs within +-256"""
    shapes = _battery_shapes()
    assert len(shapes) > 60
    worst = 0.0
    for Ni, Nj, Kc in shapes:
        if Ni * Nj * Kc > 3e10 or max(Ni, Nj) * Kc > 6e7:   # (the condition is analytic: no need to build the largest operands)
            s = Kc * 2.0 * 1.0 + 3 + 4
            assert s < 2 ** 24, (Ni, Nj, Kc)
            continue
        P, Q, bias, aux = R.operands(Ni, Nj, Kc, True)
        assert (P == P.round()).all() and (Q == Q.round()).all() and (bias == bias.round()).all() and (aux == aux.round()).all()
        assert R.conditions(P, Q, bias, aux) < 2 ** 24, (Ni, Nj, Kc)
        if Kc <= 3072 and Ni * Nj * Kc < 5e9:               # bf16-output shapes (the long contractions are weight gradients: fp32)
            r = Q.float() @ P.float().t() + bias[None, :] + aux.float()     # exact in fp32 by (1)
            frac = (r.abs() > 256).float().mean().item()
            worst = max(worst, frac)
            assert frac <= 0.01, (Ni, Nj, Kc, frac)
    print("largest fraction of outputs above 256: %.2e" % worst)
    # the heaviest bf16 case of the battery, in full
    P, Q, _, _ = R.operands(768, 2000, 3072, True)
    r = Q.float() @ P.float().t()
    assert (r.abs() > 256).float().mean().item() <= 0.01 and r.abs().max().item() < 2 ** 24
    # column sums of a stored bf16 output stay exact: sum_j |x| < 2^24 at the longest output
    assert 16400 * 512 < 2 ** 24


@pytest.mark.parametrize("Nj,Ni,K", [(130, 768, 64), (130, 768, 768), (257, 264, 3072)])
def test_emulated_kernel_arithmetic_stays_within_the_bound(Nj, Ni, K):
    worst = {}
    for block in (16, 32):
        P, Q, bias, aux = R.operands(Ni, Nj, K, False)
        for epi, f32 in ((EPI_NONE, False), (EPI_BIAS, False), (EPI_ADD, False), (EPI_DGELU, False), (EPI_BIAS_GELU, False),
                         (EPI_NONE, True), (EPI_BIAS, True)):
            out, out2 = R.emulate(P, Q, bias, aux, epi, f32, block)
            r, tol = R.bound(P, Q, bias, aux, epi, f32)
            ratio = ((out.double() - r).abs() / tol).max().item()
            worst[(epi, f32)] = max(worst.get((epi, f32), 0.0), ratio)
            assert ratio <= 1.0, (epi, f32, block, ratio)
            if out2 is not None:
                r2, tol2 = R.gelu_bound(out)
                ratio2 = ((out2.double() - r2).abs() / tol2).max().item()
                worst["gelu"] = max(worst.get("gelu", 0.0), ratio2)
                assert ratio2 <= 1.0, (block, ratio2)
                cs = out.float().sum(0)                                  # fp32 column sums of the rounded values
                rc, tc = R.colsum_bound(out)
                assert ((cs.double() - rc).abs() <= tc).all()
    print("(%d, %d, K = %d): largest |err| / bound %s" % (Nj, Ni, K, {str(k): round(v, 3) for k, v in worst.items()}))


# ---- planted defects ------------------------------------------------------------------------------------------------------------
def _defects(P, Q, bias, base):
    """name -> fp64 result (Nj, Ni) before the output rounding, wrong in ONE 64 x 64 tile (rows 64..127 / 256.., columns 128..191)"""
    Pd, Qd = P.double(), Q.double()
    K = P.shape[1]
    good = Qd @ Pd.t() + bias.double()[None, :]
    j0, i0 = 64, 128
    js, is_ = slice(j0, j0 + 64), slice(i0, i0 + 64)
    out = {}

    def variant(name):
        r = good.clone()
        out[name] = r
        return r
    r = variant("one product dropped")
    k = next(k for k in range(K) if Pd[i0 + 5, k] * Qd[j0 + 3, k] != 0)
    r[j0 + 3, i0 + 5] -= Qd[j0 + 3, k] * Pd[i0 + 5, k]
    r = variant("16-wide k slice dropped for a 32-row band")
    r[j0:j0 + 32, is_] -= Qd[j0:j0 + 32, 16:32] @ Pd[is_, 16:32].t()
    r = variant("last K tile skipped")
    r[js, is_] -= Qd[js, K - 64:] @ Pd[is_, K - 64:].t()
    r = variant("k tile added twice")
    r[js, is_] += Qd[js, :64] @ Pd[is_, :64].t()
    r = variant("two output rows swapped")
    r[[j0 + 1, j0 + 2], i0:i0 + 64] = good[[j0 + 2, j0 + 1], i0:i0 + 64]
    r = variant("ragged edge row written from the row above")
    r[-1, i0:i0 + 64] = good[-2, i0:i0 + 64]
    r = variant("k index of P and Q shifted by one")
    r[js, is_] = Qd[js, 1:] @ Pd[is_, :-1].t() + bias.double()[None, is_]
    r = variant("bias added twice")
    r[js, is_] += bias.double()[None, is_]
    return good, out


BOUND_BLIND = {"one product dropped"}   # what the bound tier cannot see at K = 3072 (real-valued operands, bf16 output)
# What the two numbers of tests/test_gemm_gpu.py::_check make of the defects, measured here at the ViT shape (16400, 768, 768)
# with the defect in one 64 x 64 tile of 3075: the relative L2 norm (<= 3e-3) accepts the first set; max |err| <= 1e-2 max |ref|
# catches every defect that moves a whole output by a few products, so both numbers together accept only the single dropped
# product.  (A skipped or doubled K tile moves the L2 norm by 5e-3 with integer operands: more than the norm allows.)
L2_ACCEPTS = {"one product dropped", "16-wide k slice dropped for a 32-row band", "ragged edge row written from the row above",
              "bias added twice"}
BOTH_ACCEPT = {"one product dropped"}


def test_what_the_old_norms_accept_at_the_vit_shape():
    P, Q, bias, _ = R.operands(768, 16400, 768, True)
    good, bad = _defects(P, Q, bias, None)
    g = R.rne_bf16(good).float()
    want = R.expected(P, Q, bias)
    l2, both = set(), set()
    for name, r in bad.items():
        out = R.rne_bf16(r)
        rel = ((out.float() - g).norm() / g.norm()).item()
        mx = ((out.float() - g).abs().max() / g.abs().max()).item()
        print("%-45s rel L2 %.2e  max %.2e  exact-tier mismatches %d" % (name, rel, mx, R.mismatches(out, want).shape[0]))
        if rel <= 3e-3:
            l2.add(name)
        if R.old_norms_accept(out, g):
            both.add(name)
        assert R.mismatches(out, want).shape[0] > 0, name
    assert l2 == L2_ACCEPTS and both == BOTH_ACCEPT, (l2, both)


@pytest.mark.parametrize("K", [768, 3072])
def test_planted_defects_fail_the_exact_tier(K):
    Nj, Ni = 257, 264
    P, Q, bias, _ = R.operands(Ni, Nj, K, True)
    good, bad = _defects(P, Q, bias, None)
    want = R.expected(P, Q, bias)
    assert R.mismatches(R.rne_bf16(good), want).shape[0] == 0
    for name, r in bad.items():
        out = R.rne_bf16(r)
        assert R.old_norms_accept(out, good) == (name in BOTH_ACCEPT), name
        n = R.mismatches(out, want).shape[0]
        assert n > 0, "%s: not seen by the exact tier" % name
    # accum overwriting instead of adding (fp32 output onto an integer base)
    base = R.int_tensor((Nj, Ni), -5, 5, "base").double()
    want32 = R.expected(P, Q, None, None, f32=True) + base
    wrong = want32.clone()
    wrong[64:128, 128:192] -= base[64:128, 128:192]
    assert R.mismatches(wrong, want32).shape[0] > 0 and R.mismatches(want32.clone(), want32).shape[0] == 0
    assert not R.old_norms_accept(wrong, want32)               # (the fp32 norms, 1e-5 / 1e-4, do see this one)
    # the same defects with real-valued operands against the bound tier
    P, Q, bias, _ = R.operands(Ni, Nj, K, False)
    good, bad = _defects(P, Q, bias, None)
    r0, tol = R.bound(P, Q, bias, None, EPI_BIAS)
    blind = set()
    for name, r in bad.items():
        out = r.float().to(torch.bfloat16).double()
        ratio = ((out - r0).abs() / tol).max().item()
        if ratio <= 1.0:
            blind.add(name)
        print("K = %d  %-45s largest |err| / bound %.2f" % (K, name, ratio))
    if K == 3072:
        assert blind == BOUND_BLIND, blind


# ---- names and routes -------------------------------------------------------------------------------------------------------------
def test_kernel_ids_parse_both_name_forms():
    assert R.kernel_ids([
        "void bq::gemm64_kernel<32, false, false, 1, false, 4, 3>(bq::GemmArgs)",
        "_ZN2bq13gemm64_kernelILi64ELb1ELb1ELi0ELb1ELi1ELi3EEEvNS_8GemmArgsE",
        "_ZN2bq17gemm64_kernel_detILi32ELb0ELb0ELi1EEEvNS_8GemmArgsE",
        "void bq::gemm128_kernel<true, false, 5, false, 16, false>(bq::GemmArgs)",
        "_ZN2bq14gemm256_kernelILb0ELb0ELi1ELb0ELb1EEEvNS_8GemmArgsE",
        "bq::splitk_fold_det_kernel(float const*, float*, __bf16*, int, int, int, int)",
        "void bq::wgrad_rows_kernel<5, 2>(bq::WgradRowsArgs)", "_ZN2bq24wgrad_rows_reduce_kernelENS_13WgradRowsArgsE",
        "void at::native::vectorized_elementwise_kernel<4>", "bq::colsum_grouped_det_kernel(bq::ColsumArgs, float*)"]) == {
        "gemm64_kernel<32,0,0,1,0,4,3>", "gemm64_kernel<64,1,1,0,1,1,3>", "gemm64_kernel_det<32,0,0,1>",
        "gemm128_kernel<1,0,5,0,16,0>", "gemm256_kernel<0,0,1,0,1>", "splitk_fold_det_kernel", "wgrad_rows_kernel<5,2>",
        "wgrad_rows_reduce_kernel"}


def _one(Ni, Nj, Kc, flags=0, epi=EPI_NONE, tile=None, **kw):
    opts = {k: kw.pop(k) for k in ("cus", "det", "streamk") if k in kw}
    ids = R.routes([dict(Ni=Ni, Nj=Nj, Kc=Kc, **kw)], flags, epi, tile, **opts)
    return ids


def test_routes_at_both_sides_of_every_threshold():
    # GEMM_TILE_ROWS and the 256-column floor of the large tiles
    assert _one(256, 1023, 128) == {"gemm64_kernel<64,0,0,0,0,1,3>"}
    assert _one(256, 1024, 128) == {"gemm128_kernel<0,0,0,0,16,0>"}
    assert _one(248, 1024, 128) == {"gemm64_kernel<64,0,0,0,0,1,3>"}
    # 32-row tiles up to 512 rows (K-contiguous Q only)
    assert _one(72, 512, 128) == {"gemm64_kernel<32,0,0,0,0,1,3>"}
    assert _one(72, 513, 128) == {"gemm64_kernel<64,0,0,0,0,1,3>"}
    assert _one(72, 64, 100, DW) == {"gemm64_kernel<64,1,1,0,1,1,3>"}
    # long_k from 12 K tiles: four K tiles per step on the 32-row tile, two on the 64-row one
    assert _one(264, 100, 64 * 11, 0, EPI_BIAS) == {"gemm64_kernel<32,0,0,1,0,1,3>"}
    assert _one(264, 100, 64 * 12, 0, EPI_BIAS) == {"gemm64_kernel<32,0,0,1,0,4,3>"}
    assert _one(264, 600, 64 * 11, 0, EPI_BIAS) == {"gemm64_kernel<64,0,0,1,0,1,3>"}
    assert _one(264, 600, 64 * 12, 0, EPI_BIAS) == {"gemm64_kernel<64,0,0,1,0,2,3>"}
    # 512 / 513 tiles: four -> two K tiles per step; 2048 / 2049: two -> one
    assert _one(64, 16384, 768, tile=32) == {"gemm64_kernel<32,0,0,0,0,4,3>"}
    assert _one(64, 16385, 768, tile=32) == {"gemm64_kernel<32,0,0,0,0,2,3>"}
    assert _one(64, 65536, 768, tile=32) == {"gemm64_kernel<32,0,0,0,0,2,3>"}
    assert _one(64, 65537, 768, tile=32) == {"gemm64_kernel<32,0,0,0,0,1,3>"}
    assert _one(64, 32 * 2048, 768, tile=64) == {"gemm64_kernel<64,0,0,0,0,2,3>"}       # 1024 tiles of 64 x 64
    # fp32 outputs and a contraction-major Q never take the long-K forms
    assert _one(264, 100, 768, OUT_F32, EPI_BIAS, 32) == {"gemm64_kernel<32,0,0,1,1,1,3>"}
    assert _one(264, 264, 1000, DW, tile=64) == {"gemm64_kernel<64,1,1,0,1,1,3>"}
    # TILE256_MIN_K: K-contiguous forward / bias launches only
    assert _one(768, 2000, 2240, 0, EPI_BIAS) == {"gemm128_kernel<0,0,1,0,16,0>"}
    assert _one(768, 2000, 2304, 0, EPI_BIAS) == {"gemm256_kernel<0,0,1,0,0>"}
    assert _one(768, 2000, 2304, P_XC) == {"gemm128_kernel<1,0,0,0,16,0>"}
    assert _one(768, 2000, 2304, 0, EPI_ADD) == {"gemm128_kernel<0,0,5,0,16,0>"}
    # tile 128 needs two K tiles, no column sums, a K-contiguous Q, bf16 out
    assert _one(256, 1024, 64) == {"gemm256_kernel<0,0,0,0,0>"}
    assert _one(3072, 16400, 768, P_XC, EPI_DGELU, colsum=True) == {"gemm256_kernel<1,0,3,0,0>"}
    assert _one(768, 2304, 16400, DW) == {"gemm256_kernel<1,1,0,1,0>"}
    # one tile class per launch: a member that cannot take tile 128 moves the group to 256
    assert R.routes([dict(Ni=768, Nj=2000, Kc=768), dict(Ni=264, Nj=1100, Kc=64)], 0, EPI_NONE) == {"gemm256_kernel<0,0,0,0,0>"}
    # a row map: 256 only for the contraction rows of the weight-gradient form, otherwise down to 64
    assert R.routes([dict(Ni=1536, Nj=16400, Kc=64, map=True)], 0, EPI_BIAS) == {"gemm64_kernel<64,0,0,1,0,1,3>"}
    assert R.routes([dict(Ni=1536, Nj=16400, Kc=768, map=True)], 0, EPI_BIAS) == {"gemm128_kernel<0,0,1,0,16,0>"}
    assert R.routes([dict(Ni=768, Nj=1536, Kc=16400, map=True)], DW, EPI_NONE) == {"gemm256_kernel<1,1,0,1,0>"}
    # more problems than one launch holds: the remainder decides its K step on its own tiles
    many = [dict(Ni=64, Nj=32 * 14, Kc=768)] * 37       # 36 x 14 = 504 tiles (four K tiles), then 14
    assert R.routes(many, 0, EPI_NONE, 32) == {"gemm64_kernel<32,0,0,0,0,4,3>"}
    many = [dict(Ni=64, Nj=32 * 15, Kc=768)] * 37       # 540 tiles (two), then 15 (four)
    assert R.routes(many, 0, EPI_NONE, 32) == {"gemm64_kernel<32,0,0,0,0,2,3>", "gemm64_kernel<32,0,0,0,0,4,3>"}
    # the deterministic mode: fp32 small-tile forms on the _det kernels, a cut contraction through the fold
    assert _one(136, 264, 9000, DW, tile=64, det=True, ksplit=8) == {"gemm64_kernel_det<64,1,1,0>", "splitk_fold_det_kernel"}
    assert _one(136, 264, 9000, DW, tile=64, det=True) == {"gemm64_kernel_det<64,1,1,0>"}
    assert _one(768, 2000, 768, 0, EPI_BIAS, det=True) == {"gemm128_kernel<0,0,1,0,16,0>"}
    assert _one(768, 2304, 16400, DW, det=True) == {"gemm256_kernel<1,1,0,1,0>"}
    # stream-K: 24 K tiles, an uneven grid, one problem, tile 128, K-contiguous operands
    assert _one(768, 16400, 3072, 0, EPI_BIAS, 128, streamk=1) == {"gemm128_kernel<0,0,1,0,16,1>"}
    assert _one(768, 16400, 3072, 0, EPI_ADD, 128, streamk=1) == {"gemm128_kernel<0,0,5,0,16,1>"}
    assert _one(768, 16400, 3072, 0, EPI_BIAS, 128, streamk=2) == {"gemm256_kernel<0,0,1,0,1>"}
    assert _one(768, 16400, 3072, 0, EPI_ADD, 128, streamk=2) == {"gemm128_kernel<0,0,5,0,16,0>"}
    assert _one(768, 16400, 3072, 0, EPI_ADD, 128, streamk=3) == {"gemm128_kernel<0,0,5,0,16,1>"}
    assert _one(768, 16400, 1472, 0, EPI_BIAS, 128, streamk=3) == {"gemm128_kernel<0,0,1,0,16,0>"}      # 23 K tiles
    assert _one(768, 16400, 3072, P_XC, EPI_NONE, 128, streamk=3) == {"gemm128_kernel<1,0,0,0,16,0>"}
    assert _one(768, 16400, 3072, BACKGROUND_ := 8, EPI_BIAS, 128, streamk=3) == {"gemm128_kernel<0,0,1,0,16,0>"}
    assert _one(768, 256 * 256, 3072, 0, EPI_BIAS, 128, streamk=2, cus=256) == {"gemm128_kernel<0,0,1,0,16,0>"}   # (an even grid)
    # the whole-row weight gradient
    assert R.wgrad_rows_routes(264, 128) == {"wgrad_rows_kernel<5,2>", "wgrad_rows_reduce_kernel"}
    assert not R.wgrad_rows_supported(328, 128) and not R.wgrad_rows_supported(64, 192) and not R.wgrad_rows_supported(320, 64)


def test_route_table_lists_each_instantiation_once():
    assert len(R.ROUTE_TABLE) == len(set(R.ROUTE_TABLE))
    assert not set(R.ROUTE_TABLE) & set(R.NOT_REACHED)
    assert sum(k.startswith("gemm64_kernel<") for k in R.ROUTE_TABLE) == 47
    assert sum(k.startswith("gemm64_kernel_det<") for k in R.ROUTE_TABLE) == 7
    assert sum(k.startswith("gemm128_kernel<") for k in R.ROUTE_TABLE) == 12
    assert sum(k.startswith("gemm256_kernel<") for k in R.ROUTE_TABLE) == 9
    assert sum(k.startswith("wgrad_rows_kernel<") for k in R.ROUTE_TABLE) == 12


# ---- the product's two statements of the routing against this reference, without a device ---------------------------------------
_GRID_NI = (8, 64, 248, 256, 264, 768, 3072)
_GRID_NJ = (1, 100, 512, 513, 1023, 1024, 16400)
_GRID_KC = (64, 127, 128, 768, 2240, 2304, 3072)
_GRID_FLAGS = (0, P_XC, OUT_F32, P_XC | OUT_F32, DW)
_GRID_EPIS = (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, R.EPI_BIAS_CE, EPI_ADD)


def _both_tiles(problems, flags, epi):
    """(product, reference) tile class of one launch; problems: (Ni, Nj, Kc, colsum, map) tuples"""
    from bridgeqa_amd import gemm_route
    got = gemm_route.auto_tile([gemm_route.Shape(*p) for p in problems], flags, epi)
    want = R.auto_tile([dict(Ni=p[0], Nj=p[1], Kc=p[2], colsum=p[3], map=p[4]) for p in problems], flags, epi)
    return got, want


def test_product_tile_policy_equals_the_reference_on_the_full_grid():
    """bridgeqa_amd/gemm_route.auto_tile (what _ext.gemm_grouped launches on) against gemm_ref.auto_tile: every threshold of
    both from both sides, all flag sets and epilogues, column sums and row maps on and off, groups of one and of two"""
    import itertools
    from bridgeqa_amd import gemm_route
    assert "gemm_route" not in vars(R) and not hasattr(gemm_route, "torch")      # (the reference stays independent; the policy pure)
    assert gemm_route.GEMM_TILE_ROWS == R.GEMM_TILE_ROWS and gemm_route.TILE256_MIN_K == [R.TILE256_MIN_K]
    n, seen = 0, set()
    for flags, epi, cs, mp in itertools.product(_GRID_FLAGS, _GRID_EPIS, (False, True), (False, True)):
        for Ni, Nj, Kc in itertools.product(_GRID_NI, _GRID_NJ, _GRID_KC):
            got, want = _both_tiles([(Ni, Nj, Kc, cs, mp)], flags, epi)
            assert got == want, ((Ni, Nj, Kc, cs, mp), flags, epi, got, want)
            seen.add(got)
            n += 1
    assert n == 7 * 7 * 7 * 5 * 6 * 4 and seen == {32, 64, 128, 256}
    # groups of two from the corners of the grid; the second member carries the column sums / the row map
    corners = list(itertools.product((_GRID_NI[0], _GRID_NI[-1]), (_GRID_NJ[0], _GRID_NJ[-1]), (_GRID_KC[0], _GRID_KC[-1])))
    for flags, epi, cs, mp in itertools.product(_GRID_FLAGS, _GRID_EPIS, (False, True), (False, True)):
        for a, b in itertools.product(corners, corners):
            got, want = _both_tiles([a + (False, False), b + (cs, mp)], flags, epi)
            assert got == want, (a, b, cs, mp, flags, epi, got, want)
    # one tile class per launch: a member with a single K tile cannot take tile 128 and moves its partner to 256 with it
    assert _both_tiles([(3072, 16400, 3072, False, False)], P_XC, EPI_NONE) == (128, 128)
    assert _both_tiles([(3072, 16400, 3072, False, False), (3072, 16400, 64, False, False)], P_XC, EPI_NONE) == (256, 256)


def test_built_library_holds_exactly_the_route_table():
    """the GEMM kernels hipcc emitted (gemm*, splitk_fold_det, wgrad_rows*: what kernel_ids() parses) are ROUTE_TABLE plus the
    GEMM ids of NOT_REACHED, no more and no fewer -- ties csrc/gemm_common.h gemm_form() to the reference table"""
    from bridgeqa_amd import build
    build.build()
    res = build.kernel_resources()
    if res is None:
        pytest.skip("objects were not compiled by this checkout's build.py (prebuilt library)")
    built = R.kernel_ids(res)
    want = set(R.ROUTE_TABLE) | R.kernel_ids(R.NOT_REACHED)
    assert built == want, {"not in the table": sorted(built - want), "not built": sorted(want - built)}


@pytest.mark.parametrize("epi", [-1, 6, 99])
def test_library_refuses_an_epilogue_outside_the_enum(epi):
    """bq_gemm_bf16 checks the epilogue before it reads a descriptor (null here: nothing can be launched)"""
    from bridgeqa_amd import _ext
    assert _ext._lib.bq_gemm_bf16(None, 0, 0, epi, 64, None) == _ext._D["BQ_EINVAL"]
    msg = _ext._lib.bq_last_error()
    assert b"epilogue" in msg and str(epi).encode() in msg, msg
