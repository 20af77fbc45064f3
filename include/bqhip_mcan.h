/* bqhip_mcan.h -- the two row operators of the MCAN blocks (csrc/mcan.hip): MCAN's own residual LayerNorm and AttFlat's masked
 * softmax pooling, forward and backward.  Additive to ABI 6: bqhip_fusion.h includes this file, BQHIP_ABI_VERSION does not move,
 * no existing entry point changes.  Same conventions as bqhip_lstm.h (raw device pointers, extents, a hipStream_t passed as
 * void*, int status, bq_last_error(); BQ_EINVAL and nothing launched for an ineligible size or a null pointer).
 *
 * fp32 throughout, no atomics, every sum in a fixed order: two runs give the same bits.  Nothing allocates or synchronises.
 *
 * Residual LayerNorm (reference models/mcan_module.py:57-69 applied to x + s).  M rows of H values, H a multiple of 64 in
 * [64, 1024]; one wave per row.  Per row, every operation rounded to fp32 in this order:
 *   z = x + s (s NULL: z = x),  mean = (sum_j z) / H,  c = z - mean,  sigma = sqrtf((sum_j c c) / (H - 1)),
 *   r = 1 / (sigma + eps),  q = c r,  y = a2 q + b2.
 * The UNBIASED deviation, and eps added to sigma, not to the variance.  sigma = 0 is not guarded: y = b2 there.
 * bqm_mcan_ln_fwd writes y (M, H), mean (M), sigma (M).
 * bqm_mcan_ln_bwd takes mean and sigma as saved and re-forms z, c, r, q as above; g = dy a2, s1 = (sum_j g) / H,
 *   s2 = sum_j g c, k = (r r) / ((H - 1) sigma), dz = r (g - s1) - (k s2) c: the gradient of x AND of s (one tensor);
 *   dab (2, H) = [sum_rows dy q, sum_rows dy] is STORED (not accumulated): every workgroup stores its partial to `slab`
 *   (bqm_mcan_ln_bwd_slab_floats(M, H) floats) and a second launch adds the partials in a fixed (tree) order.
 *   A row with sigma = 0 gets NaN in dz (inf 0), as autograd of the composition gives.
 *
 * AttFlat pool (reference models/mcan_module.py:113-133 after the MLP): x (B, N, H), logits (B, N, G), hide (B, N) bytes
 * (non-zero = hidden key) or NULL; 1 <= G <= 4, 1 <= N <= 1024, H a multiple of 64 up to 1024.
 *   l = hide ? -1e9f : logit (a FILL, not -inf: a fully hidden sample pools uniformly, 1 / N),  p = softmax over n with the
 *   maximum subtracted and expf,  out[b][g H + h] = sum_n p[b][n][g] x[b][n][h] added in ascending n.
 * bqm_attflat_pool_fwd writes out (B, G H) and p (B, N, G).
 * bqm_attflat_pool_bwd: dx[b][n][h] = sum_g p dout (ascending g),  da[b][n][g] = sum_h x dout,  t = sum_n p da,
 *   dlogits = hide ? 0 : p (da - t)   (masked_fill passes no gradient; p is 1 / N, not 0, under a full mask).
 *
 * The entry points are named bqm_: the bq_ symbols and the bqx_ symbols of the library are both closed censuses
 * (tests/test_cabi_cpu.py and tests/test_beam_device_cpu.py count them); this family carries a prefix of its own and is derived
 * (bridgeqa_amd/_cabi.py MCAN_PROTOS) and compiled against this declaration like every other entry point. */
#ifndef BQHIP_MCAN_H
#define BQHIP_MCAN_H
#include "bqhip.h"

#define BQ_MCAN_MAX_H 1024
#define BQ_MCAN_MAX_N 1024
#define BQ_MCAN_MAX_G 4
#define BQ_MCAN_LN_BWD_CAP 256

#ifdef __cplusplus
extern "C" {
#endif

BQ_API int bqm_mcan_ln_fwd(const float *x, const float *s, const float *a2, const float *b2, float *y, float *mean,
                           float *sigma, int M, int H, float eps, void *stream);
BQ_API long bqm_mcan_ln_bwd_slab_floats(int M, int H);
BQ_API int bqm_mcan_ln_bwd(const float *dy, const float *x, const float *s, const float *a2, const float *mean,
                           const float *sigma, float *dz, float *dab, float *slab, int M, int H, float eps, void *stream);
BQ_API int bqm_attflat_pool_fwd(const float *x, const float *logits, const unsigned char *hide, float *out, float *p, int B,
                                int N, int G, int H, void *stream);
BQ_API int bqm_attflat_pool_bwd(const float *dout, const float *x, const float *p, const unsigned char *hide, float *dx,
                                float *dlogits, int B, int N, int G, int H, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_MCAN_H */
