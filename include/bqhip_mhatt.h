/* bqhip_mhatt.h -- the attention core of the MCAN blocks' MHAtt (csrc/mhatt.hip): scores, fill, softmax, dropout multiplier, the
 * product with V, and their backward.  Additive to ABI 6: bqhip_fusion.h includes this file, BQHIP_ABI_VERSION does not move, no
 * existing entry point changes.  Same conventions as bqhip_mcan.h (raw device pointers, extents, a hipStream_t passed as void*,
 * int status, bq_last_error(); BQ_EINVAL and nothing launched for an ineligible size -- checked before any pointer is looked at
 * -- or a null pointer; B == 0 is BQ_OK).
 *
 * fp32 throughout, no atomics, every sum in ONE order: two runs give the same bits.  Nothing allocates or synchronises.
 *
 * Operands.  q (B, Nq, heads d), k and v (B, Nk, heads d): the outputs of linear_q / linear_k / linear_v as they stand, read in
 * place -- head h of a row is its columns [h d, (h + 1) d); no head-split transpose, no copy.  hide (B, Nk) bytes, non-zero =
 * hidden key, or NULL.  keep (B, heads, Nq, Nk): the dropout multiplier, 0 or 1 / (1 - p_drop), or NULL.
 * Eligible: d in {32, 64}, heads >= 1, 1 <= Nq, Nk <= BQ_MHATT_MAX_N, B heads <= 65535 (a grid extent).
 *
 * Forward (reference models/mcan_module.py:206-224), per (sample b, head h); every operation rounded to fp32, in this order:
 *   a_ij = sum_c q_ic k_jc            one product per term, added to a chain that starts at 0, for ascending c
 *   s_ij = a_ij / sqrtf(d)            a division by the fp32 value
 *   l_ij = hide[b][j] ? -1e9f : s_ij  a FILL, not -inf: a query whose keys are all hidden attends uniformly, 1 / Nk
 *   m_i = max_j l_ij,  e_ij = expf(l_ij - m_i),  z_i = sum_j e_ij,  p_ij = e_ij / z_i
 *                                     z: lane n of a wave adds its keys j = n, n + 64, ... for ascending j, starting at 0, and
 *                                     the 64 lane sums are folded by the xor butterfly 32, 16, .. 1 (halves added)
 *   w_ij = p_ij keep_ij               (keep NULL: w = p)
 *   out_ic = sum_j w_ij v_jc          one product per term, a chain from 0 for ascending j
 * bqh_mhatt_fwd writes out (B, Nq, heads d) -- the layout linear_merge reads; there is no transpose().contiguous() -- and
 * p (B, heads, Nq, Nk), the probabilities BEFORE the dropout multiplier, which the backward reads.
 *
 * Backward (p is read as saved; q, k, v, hide, keep as in the forward; dout (B, Nq, heads d)):
 *   g_ij  = sum_c dout_ic v_jc        a chain from 0 for ascending c
 *   dp_ij = keep_ij g_ij              (keep NULL: dp = g)
 *   t_i   = sum_j p_ij dp_ij          lanes and butterfly as z above
 *   ds_ij = hide[b][j] ? 0 : p_ij (dp_ij - t_i)      masked_fill passes no gradient, and under a full mask p is 1 / Nk, not 0
 *   dq_ic = (sum_j ds_ij k_jc) / sqrtf(d)            a chain from 0 for ascending j
 *   dk_jc = (sum_i ds_ij q_ic) / sqrtf(d)            a chain from 0 for ascending i
 *   dv_jc = sum_i (p_ij keep_ij) dout_ic             a chain from 0 for ascending i; p keep is formed again, one rounding
 * bqh_mhatt_bwd writes dq (B, Nq, heads d), dk and dv (B, Nk, heads d); every element is STORED once (nothing accumulates into
 * the outputs).  Two launches: the query-major pass forms g, dp, t, ds, writes dq and stores ds to the workspace `ws`
 * (B, heads, Nq, Nk) -- bqh_mhatt_bwd_ws_floats floats, 0 for an ineligible size; the key-major pass reads it back, one lane
 * per key with its d + d accumulators in registers, no cross-lane reduction.
 *
 * The entry points are named bqh_: the bq_, bqx_ and bqm_ symbols of the library are closed censuses (tests/test_cabi_cpu.py,
 * tests/test_beam_device_cpu.py, tests/test_mcan_rows_cpu.py); this family carries a prefix of its own and is derived
 * (bridgeqa_amd/_cabi.py MHATT_PROTOS) and compiled against this declaration like every other entry point. */
#ifndef BQHIP_MHATT_H
#define BQHIP_MHATT_H
#include "bqhip.h"

#define BQ_MHATT_MAX_N 1024

#ifdef __cplusplus
extern "C" {
#endif

BQ_API int bqh_mhatt_fwd(const float *q, const float *k, const float *v, const unsigned char *hide, const float *keep,
                         float *out, float *p, int B, int heads, int Nq, int Nk, int d, void *stream);
BQ_API long bqh_mhatt_bwd_ws_floats(int B, int heads, int Nq, int Nk, int d);
BQ_API int bqh_mhatt_bwd(const float *dout, const float *q, const float *k, const float *v, const float *p,
                         const unsigned char *hide, const float *keep, float *dq, float *dk, float *dv, float *ws, int B,
                         int heads, int Nq, int Nk, int d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_MHATT_H */
