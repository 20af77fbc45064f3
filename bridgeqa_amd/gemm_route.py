"""Which tile class a launch of the MFMA bf16 GEMM family gets (which kernel forms exist: gemm_form(), csrc/gemm_common.h).
Pure -- neither torch nor the library -- so tests/test_gemm_bound_cpu.py can hold it to tests/gemm_ref.py on plain numbers."""
from collections import namedtuple

from ._cabi import DEFINES as _D

P_XC, Q_XC, OUT_F32 = (_D["BQ_GEMM_" + n] for n in ("P_XC", "Q_XC", "OUT_F32"))
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_ADD = (_D["BQ_GEMM_EPI_" + n] for n in ("NONE", "BIAS", "BIAS_GELU", "DGELU", "ADD"))

# what the policy reads of one problem: row_map = Q or out is a batched-row view (q_rpb / o_rpb of bq_gemm_desc)
Shape = namedtuple("Shape", "Ni Nj Kc colsum row_map")

GEMM_TILE_ROWS = 1024  # problems with at least this many j rows (and i columns >= 256) run on the large-tile kernels
# forward / dX launches (K-contiguous operands, plain or bias epilogue) whose contraction is at least this long run on the
# 256 x 256 kernel instead of the 256 x 128 one: since round 6's K loop it is level or ahead alone (fc2 forward 71 against
# 77 us) and inside the c3 step (31.81 against 32.05 ms: DESIGN.md 4.4, profiles/r06_tile256_long_k.txt).
# 0 = never (tools/ab_bench.py "_ext.TILE256_MIN_K[0]=0")
TILE256_MIN_K = [2304]


def pick_tile(Ni, Nj, q_xc):
    if Nj >= GEMM_TILE_ROWS and Ni >= 256:
        return 128
    if q_xc or Nj > 512:  # (64-row tiles from 100 / 200 rows up: measured 0.3-0.4 ms SLOWER per c3 step)
        return 64
    return 32


def auto_tile(shapes, flags, epilogue):
    """the tile class of one launch (one class per launch) over `shapes`, when the caller names none"""
    pxc, qxc, f32 = bool(flags & P_XC), bool(flags & Q_XC), bool(flags & OUT_F32)
    t = max([32] + [pick_tile(s.Ni, s.Nj, qxc) for s in shapes])
    # Large problems whose output is bf16 with a K-contiguous Q (forward, input gradient) take the 256 x 128 persistent kernel
    # (csrc/gemm_mid.hip: round 3 A/B against the 256 x 256 one: 38.8 vs 39.2 ms per c3 step) when EVERY problem of the group
    # can; its weight-gradient form (tile=128 on request) measured slower inside the step and is never the automatic choice
    mid_ok = (not qxc and not f32 and epilogue in (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_ADD)
              and all(s.Kc >= 128 and not s.colsum for s in shapes))
    if t == 128 and not mid_ok:
        t = 256
    if (t == 128 and TILE256_MIN_K[0] and not pxc and epilogue in (EPI_NONE, EPI_BIAS)
            and all(s.Kc >= TILE256_MIN_K[0] for s in shapes)):
        t = 256   # (long contractions: TILE256_MIN_K above)
    if t == 256 and any(s.row_map for s in shapes) and not (pxc and qxc and f32):
        t = 64    # (the 256 x 256 kernel maps only the contraction rows of its weight-gradient form)
    return t


# ---- weight gradients (fusion_wgrad.py, fusion_ops.py): dW = dY^T X, contraction over the rows ------------------------------------
BIG_ROWS = 1024  # contractions at least this long run on the 256 x 256 kernel (measured: sending the text side's 160-640-row
                 # contractions there too costs +1.5 ms per c3 step -- its pipeline fill and 256 KB fp32 tile epilogue dominate)
DW_TILE = [256]   # big: 256 = gemm256_kernel (one workgroup per CU); 128 = the 256 x 128 persistent kernel's weight-gradient form
SHORT_DW_MIN_ROWS = [64]    # mid: contractions from this many rows on (the decoder's B x 5 answer rows = 80 included: the flush
                            # 0.53 -> 0.48 ms, bit-identical; the 256 x 128 form, SHORT_DW_TILE = 128, needs >= 128)
SHORT_DW_TILE = [256]  # mid (short contractions, rows < 1024: the text side's B x 20 token rows): 256 = gemm256_kernel (since
                       # round 6's K loop: the 228 problems of one flush 0.52 ms against 0.59 on the persistent 256 x 128
                       # kernel's weight-gradient form and 0.77 on the 64 x 64-tile kernel, tools/bench_short_dw.py,
                       # bit-identical results; c3 step 31.31 -> 31.17 ms, profiles/r06_short_dw_tile.txt); 128 and 64 select those


def wgrad_class(rows, parked=None):
    """'big' (DW_TILE), 'mid' (SHORT_DW_TILE) or 'small' (the 64 x 64-tile kernel) for a weight gradient over `rows` rows.
    parked: (dY columns, X columns, dY is plain 2-D rows) of a record of the deferred flush -- only those have a mid class"""
    if rows >= BIG_ROWS:
        return "big"
    if parked is not None and SHORT_DW_TILE[0] in (128, 256):
        n_out, n_in, plain = parked
        if rows >= max(SHORT_DW_MIN_ROWS[0], 128 if SHORT_DW_TILE[0] == 128 else 1) and plain and n_out >= 128 and n_in >= 256:
            return "mid"
    return "small"
