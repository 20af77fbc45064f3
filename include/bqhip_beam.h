/* bqhip_beam.h -- one beam-search step on the device (csrc/beam.hip): candidate scores, the top 2 nb of every sample, the open
 * beams, the finished-hypothesis heaps and the reorder of the token and ancestry tables.  Additive to ABI 6: bqhip_fusion.h
 * includes this file, BQHIP_ABI_VERSION does not move, no existing entry point changes.  Same conventions as bqhip.h (raw
 * device pointers, a hipStream_t passed as void*, int status, bq_last_error()).
 *
 * Restates one iteration of generation.beam_search (bridgeqa_amd/generation.py) for B samples x nb beams (S = B nb slots) after
 * the decoder wrote the step's logits (S, V).  cur_len = *pos is read on the DEVICE, so a captured step replays.
 *
 *   score(r, v) = beam_score[r] + ((x[r][v] - max_v x[r]) - logf(sum_v expf(x[r][v] - max_v x[r])))         all fp32
 *   (eos: -inf before the add while cur_len < min_length; a NaN or +inf logit makes its whole row NaN, as log_softmax does)
 *
 * THE ORDER over the nb V scores of a sample is total and part of the ABI: score descending, a NaN above every number,
 * -0 equal to +0, equal scores by ascending flat index r_local V + v.  The first 2 nb candidates of that order are the
 * step's candidates (top_score / top_index, rank order).  The first nb non-eos candidates become the next beams; the eos
 * candidates among the first nb ranks go to the sample's heap as BeamHypotheses.add does it, in double:
 *   score = (double)sum_logprobs / lenpow[cur_len]; append when the heap holds fewer than nb entries or score > worst; with
 *   nb + 1 entries the first entry of lowest score leaves and worst becomes the new lowest score; else worst = min(score, worst).
 * The heap keeps list order through heap_seq (the number of the add that stored the entry): a smaller number is earlier in the
 * list; physical rows are reused.  is_done: heap full and (early_stopping or worst >= (double)rank-0 score / lenpow[cur_len]).
 * A done sample gets next scores 0, next tokens pad, source slots the identity, and its heap is not touched again.
 *
 * State update (all in place; every sample belongs to ONE workgroup, which reads the sample's token rows and ancestry columns
 * completely before it writes any of them): tokens[s][0 .. cur_len) = old tokens[src[s]], tokens[s][cur_len] = next token;
 * anc[j][s] = old anc[j][src[s]] for j < cur_len, anc[cur_len][s] = s when cur_len < Lmax; beam_score; ids; done; src;
 * not_done[0] = samples not yet done, not_done[1 + cur_len] = the same (a history the host may read late).
 * A step with cur_len outside [1, max_length) writes nothing.
 *
 * Three launches: rows (S workgroups), samples (B workgroups), count (1).  No float atomics: every sum and every selection has
 * a fixed order.  Nothing allocates, synchronises or copies to the host.
 * Limits: 1 <= nb <= BQ_BEAM_MAX_NB, 2 nb <= V, nb V < 2^31, max_length <= BQ_BEAM_MAX_LEN, Lmax <= BQ_BEAM_MAX_LEN, eos and
 * pad in [0, V).  Bad extents or a null pointer: BQ_EINVAL and a bq_last_error() text, nothing is launched.
 *
 * The entry point is named bqx_: the bq_ symbols of the library are a closed census (tests/test_cabi_cpu.py counts them), and
 * what is added after it carries this prefix.  Declared, derived (bridgeqa_amd/_cabi.py EXTENSION_PROTOS) and compiled against
 * this declaration like every bq_ entry point. */
#ifndef BQHIP_BEAM_H
#define BQHIP_BEAM_H
#include "bqhip.h"

#define BQ_BEAM_MAX_NB 16
#define BQ_BEAM_MAX_LEN 64
#define BQ_BEAM_THREADS 512

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bq_beam_state {
  int B, nb, V, max_length, Lmax, eos, pad, min_length, early_stopping, logits_bf16;
  long ld_logits;            /* elements between two rows of logits */
  const void *logits;        /* (S, V) float, or bf16 when logits_bf16 != 0 */
  const int32_t *pos;        /* (1) cur_len */
  const double *lenpow;      /* (max_length + 1) n ** length_penalty */
  float *beam_score;         /* (S) */
  int32_t *tokens;           /* (S, max_length) */
  int32_t *anc;              /* (Lmax, S) */
  long long *ids;            /* (S) the token the next decoder step reads */
  int32_t *done;             /* (B) */
  int32_t *not_done;         /* (1 + BQ_BEAM_MAX_LEN + 1) */
  int32_t *src;              /* (S) source slot of every new beam */
  long long *cand;           /* (S, 2 nb) scratch between the row and the sample launch */
  float *top_score;          /* (B, 2 nb) */
  int32_t *top_index;        /* (B, 2 nb) flat index r_local V + v */
  int32_t *heap_len;         /* (B) */
  int32_t *heap_adds;        /* (B) adds stored so far */
  int32_t *heap_seq;         /* (B, nb) */
  int32_t *heap_hyplen;      /* (B, nb) */
  float *heap_sum;           /* (B, nb) sum_logprobs */
  double *heap_score;        /* (B, nb) */
  double *heap_worst;        /* (B) */
  int32_t *heap_tokens;      /* (B, nb, max_length) */
} bq_beam_state;

BQ_API int bqx_beam_step(const bq_beam_state *st, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_BEAM_H */
