/* bqhip_lstm.h -- the LSTM recurrence of the question branch (csrc/lstm.hip).  Additive to ABI 6: bqhip_fusion.h includes
 * this file, BQHIP_ABI_VERSION does not move, no existing entry point changes.  Same conventions as bqhip.h (raw device
 * pointers, extents, a hipStream_t passed as void*, int status, bq_last_error()).
 *
 * Replaces the recurrence of nn.LSTM over a packed sequence (reference models/lang_module.py:48-55, 95-99) for ONE layer and
 * ONE direction; fp32 throughout; H in {128, 256} (anything else: BQ_EINVAL).  One workgroup per sequence, no communication
 * between workgroups, no atomics: two runs give the same bits.
 *
 * bq_lstm_fwd: Gx (B, T, 4H) = x W_ih^T + b_ih + b_hh for every step (gate order i f g o); WT (H, 4H) = W_hh^T; lens (B) int32,
 *   clamped to [0, T_out] in the kernel; T_out <= T.  Writes Y (B, T_out, H) -- rows t >= lens[b] as ZEROS, no memset needed --
 *   and h_last (B, H): the state after step lens[b] - 1 (reverse != 0: the steps run lens[b] - 1 .. 0 and h_last is the state
 *   after step 0); zero initial state.  gates (B, T_out, 4H) / cells (B, T_out, H): both NULL, or both written for t < lens[b]
 *   (post-activation gates, cell states: what bq_lstm_bwd reads; rows t >= lens[b] are left untouched).
 * bq_lstm_bwd: dY (B, T_out, H) or NULL, dh_last (B, H) or NULL, gates / cells as saved, W (4H, H) = W_hh as nn.LSTM holds it.
 *   Writes dGx (B, T_out, 4H), the gradient of the pre-activation gates, rows t >= lens[b] as zeros.  dX, dW_ih, dW_hh and the
 *   bias gradients are matrix products / a column sum over dGx. */
#ifndef BQHIP_LSTM_H
#define BQHIP_LSTM_H
#include "bqhip.h"

#ifdef __cplusplus
extern "C" {
#endif

BQ_API int bq_lstm_fwd(const float *Gx, const float *WT, const int32_t *lens, float *Y, float *h_last, float *gates,
                       float *cells, int B, int T, int T_out, int H, int reverse, void *stream);
BQ_API int bq_lstm_bwd(const float *dY, const float *dh_last, const float *gates, const float *cells, const float *W,
                       const int32_t *lens, float *dGx, int B, int T_out, int H, int reverse, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_LSTM_H */
