// One beam-search step on the device (include/bqhip_beam.h states the semantics, the total order and the state update).
//
//   beam_rows_kernel    one workgroup per slot r: max, sum exp, then the row's first 2 nb candidates of THE ORDER
//   beam_sample_kernel  one workgroup per sample: merge the nb rows' candidates, open beams, heaps, done, reorder
//   beam_count_kernel   samples not yet done
//
// A candidate is one u64 whose unsigned order is THE ORDER: (monotone image of the fp32 score) << 32 | (2^31 - 1 - flat index);
// 0 is "none".  The top 2 nb of a sample lie among the top 2 nb of each of its rows, so the row kernel may select per row.
// Row selection: every thread keeps the best key of ITS elements below the previous winner; after a round only the thread that
// owned the winner scans its elements again (the others' bests are still valid), so a round costs one workgroup max.
// The logits were just written by the LM head: the three reads of a row come from L2.
#include "bq_common.h"

namespace bq {

constexpr int BEAM_NT = BQ_BEAM_THREADS;
constexpr int BEAM_WAVES = BEAM_NT / 64;
constexpr int BEAM_K2 = 2 * BQ_BEAM_MAX_NB;
typedef unsigned long long u64;

__device__ __forceinline__ unsigned beam_ord(float s) {
  if (s != s) return 0xFFFFFFFFu;
  unsigned b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;   // -0 is +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float beam_unord(unsigned o) {
  if (o == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ u64 beam_key(float s, int flat) { return ((u64)beam_ord(s) << 32) | (u64)(0x7FFFFFFF - flat); }

__device__ __forceinline__ float load_f(const float *p) { return *p; }
__device__ __forceinline__ float load_f(const __bf16 *p) { return (float)*p; }

// f(v, x) for every element of the row; a thread's elements in a fixed order: its head element (before the first 16-byte
// boundary), its 16-byte vectors (vector i of the row belongs to thread i % BEAM_NT), its tail element
template <class F>
__device__ __forceinline__ void row_each(const float *row, int V, F &&f) {
  const int tid = threadIdx.x;
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / 4u);
  head = head < V ? head : V;
  const int nvec = (V - head) / 4;
  if (tid < head) f(tid, row[tid]);
  const float4 *rv = (const float4 *)(row + head);
  for (int i = tid; i < nvec; i += BEAM_NT) {
    const float4 x = rv[i];
    const int v = head + 4 * i;
    f(v, x.x); f(v + 1, x.y); f(v + 2, x.z); f(v + 3, x.w);
  }
  const int tail = head + 4 * nvec;
  if (tail + tid < V) f(tail + tid, row[tail + tid]);
}
template <class F>
__device__ __forceinline__ void row_each(const __bf16 *row, int V, F &&f) {
  const int tid = threadIdx.x;
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / 2u);
  head = head < V ? head : V;
  const int nvec = (V - head) / 8;
  if (tid < head) f(tid, load_f(row + tid));
  const uint4 *rv = (const uint4 *)(row + head);
  for (int i = tid; i < nvec; i += BEAM_NT) {
    const uint4 x = rv[i];
    const int v = head + 8 * i;
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(v + 2 * j, __uint_as_float(w[j] << 16));
      f(v + 2 * j + 1, __uint_as_float(w[j] & 0xFFFF0000u));
    }
  }
  const int tail = head + 8 * nvec;
  if (tail + tid < V) f(tail + tid, load_f(row + tail + tid));
}

__device__ __forceinline__ float wave_all_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// butterfly: every level adds the same two values in both lanes of a pair, so all lanes end with the same bits
__device__ __forceinline__ float wave_all_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ u64 wave_all_max(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), o), lo = (unsigned)__shfl_xor((int)(unsigned)v, o);
    const u64 w = ((u64)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

template <class T>
__global__ __launch_bounds__(BEAM_NT) void beam_rows_kernel(bq_beam_state st) {
  __shared__ float red_f[2][BEAM_WAVES];
  __shared__ u64 red_k[2][BEAM_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const int V = st.V, K2 = 2 * st.nb;
  const int cur_len = st.pos[0];
  if (cur_len < 1 || cur_len >= st.max_length) return;
  const T *row = (const T *)st.logits + (long)r * st.ld_logits;
  const float bs = st.beam_score[r];
  const int no_eos = cur_len < st.min_length ? st.eos : -1;
  const int flat0 = (r % st.nb) * V;

  float m = -INFINITY;
  row_each(row, V, [&](int, float x) { m = fmaxf(m, x); });
  m = wave_all_max(m);
  if ((tid & 63) == 0) red_f[0][wave] = m;
  __syncthreads();
  m = red_f[0][0];
#pragma unroll
  for (int w = 1; w < BEAM_WAVES; ++w) m = fmaxf(m, red_f[0][w]);

  float sum = 0.f;
  row_each(row, V, [&](int, float x) { sum = sum + expf(x - m); });
  sum = wave_all_sum(sum);
  if ((tid & 63) == 0) red_f[1][wave] = sum;
  __syncthreads();
  sum = red_f[1][0];
#pragma unroll
  for (int w = 1; w < BEAM_WAVES; ++w) sum = sum + red_f[1][w];
  const float lse = logf(sum);

  u64 prev = ~0ull, mine = ~0ull;
  for (int k = 0; k < K2; ++k) {
    if (mine == prev) {   // (round 0: everybody) the owner of the last winner looks for its next one
      u64 best = 0;
      row_each(row, V, [&](int v, float x) {
        const float lp = v == no_eos ? -INFINITY : (x - m) - lse;
        const u64 key = beam_key(bs + lp, flat0 + v);
        if (key < prev && key > best) best = key;
      });
      mine = best;
    }
    const u64 wmax = wave_all_max(mine);
    if ((tid & 63) == 0) red_k[k & 1][wave] = wmax;
    __syncthreads();
    u64 win = red_k[k & 1][0];
#pragma unroll
    for (int w = 1; w < BEAM_WAVES; ++w) win = red_k[k & 1][w] > win ? red_k[k & 1][w] : win;
    if (tid == 0) st.cand[(long)r * K2 + k] = (long long)win;
    if (win == 0) {   // fewer than 2 nb elements (uniform): the rest is "none"
      for (int j = k + 1 + tid; j < K2; j += BEAM_NT) st.cand[(long)r * K2 + j] = 0;
      break;
    }
    prev = win;
  }
}

__global__ __launch_bounds__(BEAM_NT) void beam_sample_kernel(bq_beam_state st) {
  __shared__ u64 keys[BQ_BEAM_MAX_NB * BEAM_K2];
  __shared__ u64 sorted[BEAM_K2];
  __shared__ int tok[BQ_BEAM_MAX_NB][BQ_BEAM_MAX_LEN];
  __shared__ int anc_l[BQ_BEAM_MAX_LEN][BQ_BEAM_MAX_NB];
  __shared__ float open_score[BQ_BEAM_MAX_NB];
  __shared__ int open_tok[BQ_BEAM_MAX_NB], open_src[BQ_BEAM_MAX_NB];
  __shared__ int add_row[BQ_BEAM_MAX_NB], add_src[BQ_BEAM_MAX_NB];
  __shared__ int n_add, now_done;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = st.nb, V = st.V, K2 = 2 * nb, ML = st.max_length, S = st.B * nb, s0 = b * nb;
  const int cur_len = st.pos[0];
  if (cur_len < 1 || cur_len >= ML) return;
  const int n_anc = cur_len < st.Lmax ? cur_len : st.Lmax;

  // ---- read everything of the sample that is rewritten below
  const int n_keys = nb * K2;
  if (tid < n_keys) keys[tid] = (u64)st.cand[(long)s0 * K2 + tid];
  if (tid < K2) sorted[tid] = 0;
  for (int i = tid; i < nb * cur_len; i += BEAM_NT) tok[i / cur_len][i % cur_len] = st.tokens[(long)(s0 + i / cur_len) * ML + i % cur_len];
  for (int i = tid; i < n_anc * nb; i += BEAM_NT) anc_l[i / nb][i % nb] = st.anc[(long)(i / nb) * S + s0 + i % nb];
  const int was_done = st.done[b];
  __syncthreads();

  // ---- the sample's first 2 nb candidates: rank = keys above mine (all keys differ: the flat index is part of them)
  if (tid < n_keys) {
    const u64 k = keys[tid];
    int rank = 0;
    for (int j = 0; j < n_keys; ++j) rank += keys[j] > k;
    if (k != 0 && rank < K2) sorted[rank] = k;
  }
  __syncthreads();
  if (tid < K2) {
    const u64 k = sorted[tid];
    st.top_score[b * K2 + tid] = beam_unord((unsigned)(k >> 32));
    st.top_index[b * K2 + tid] = k ? 0x7FFFFFFF - (int)(unsigned)k : -1;
  }

  // ---- BeamSearchScorer.process of one sample, serial
  if (tid == 0) {
    int adds = 0, done = was_done;
    for (int i = 0; i < nb; ++i) {
      open_score[i] = 0.f;
      open_tok[i] = st.pad;
      open_src[i] = i;
    }
    if (!done) {
      const double lp = st.lenpow[cur_len];
      int len = st.heap_len[b];
      double worst = st.heap_worst[b];
      int n_open = 0;
      for (int j = 0; j < K2; ++j) {
        const u64 k = sorted[j];
        const long flat = 0x7FFFFFFF - (long)(unsigned)k;
        if (k == 0 || flat >= (long)nb * V) continue;
        const float s = beam_unord((unsigned)(k >> 32));
        const int beam = (int)(flat / V), t = (int)(flat % V);
        if (t == st.eos) {
          if (j >= nb) continue;
          const double sc = (double)s / lp;
          if (!(len < nb || sc > worst)) continue;
          int rowi = -1;
          if (len < nb) {
            rowi = len++;
            worst = worst < sc ? worst : sc;
          } else {   // nb + 1 entries: the first entry of lowest score leaves, worst = the new lowest
            int e = 0;
            for (int i = 1; i < nb; ++i) {
              const double a = st.heap_score[b * nb + i], c = st.heap_score[b * nb + e];
              if (a < c || (a == c && st.heap_seq[b * nb + i] < st.heap_seq[b * nb + e])) e = i;
            }
            if (sc < st.heap_score[b * nb + e]) {
              worst = st.heap_score[b * nb + e];   // the new entry itself leaves
            } else {
              rowi = e;
              worst = sc;
              for (int i = 0; i < nb; ++i)
                if (i != e && st.heap_score[b * nb + i] < worst) worst = st.heap_score[b * nb + i];
            }
          }
          if (rowi >= 0) {
            st.heap_score[b * nb + rowi] = sc;
            st.heap_sum[b * nb + rowi] = s;
            st.heap_hyplen[b * nb + rowi] = cur_len;
            st.heap_seq[b * nb + rowi] = st.heap_adds[b] + adds;
            add_row[adds] = rowi;
            add_src[adds] = beam;
            ++adds;
          }
        } else if (n_open < nb) {
          open_score[n_open] = s;
          open_tok[n_open] = t;
          open_src[n_open] = beam;
          ++n_open;
        }
      }
      st.heap_len[b] = len;
      st.heap_worst[b] = worst;
      st.heap_adds[b] += adds;
      const float best = beam_unord((unsigned)(sorted[0] >> 32));
      done = len >= nb && (st.early_stopping || worst >= (double)best / lp);
      if (done)
        for (int i = 0; i < nb; ++i) {
          open_score[i] = 0.f;
          open_tok[i] = st.pad;
          open_src[i] = i;
        }
    }
    n_add = adds;
    now_done = done;
  }
  __syncthreads();

  // ---- the finished hypotheses' tokens (a thread owns a column and writes the adds in order: a row reused twice ends right)
  if (tid < cur_len)
    for (int a = 0; a < n_add; ++a) st.heap_tokens[((long)b * nb + add_row[a]) * ML + tid] = tok[add_src[a]][tid];
  // ---- the reorder, from the copies in LDS
  for (int i = tid; i < nb * (cur_len + 1); i += BEAM_NT) {
    const int s = i / (cur_len + 1), j = i % (cur_len + 1);
    st.tokens[(long)(s0 + s) * ML + j] = j < cur_len ? tok[open_src[s]][j] : open_tok[s];
  }
  for (int i = tid; i < n_anc * nb; i += BEAM_NT) st.anc[(long)(i / nb) * S + s0 + i % nb] = anc_l[i / nb][open_src[i % nb]];
  if (tid < nb) {
    if (cur_len < st.Lmax) st.anc[(long)cur_len * S + s0 + tid] = s0 + tid;
    st.beam_score[s0 + tid] = open_score[tid];
    st.ids[s0 + tid] = open_tok[tid];
    st.src[s0 + tid] = s0 + open_src[tid];
  }
  if (tid == 0) st.done[b] = now_done;
}

__global__ __launch_bounds__(64) void beam_count_kernel(bq_beam_state st) {
  const int cur_len = st.pos[0];
  if (cur_len < 1 || cur_len >= st.max_length) return;
  int n = 0;
  for (int b = threadIdx.x; b < st.B; b += 64) n += st.done[b] == 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
  if (threadIdx.x == 0) {
    st.not_done[0] = n;
    st.not_done[1 + cur_len] = n;
  }
}

}  // namespace bq

extern "C" int bqx_beam_step(const bq_beam_state *stp, void *stream) {
  using namespace bq;
  BQ_REQUIRE(stp, BQ_EINVAL, "beam_step: null state");
  const bq_beam_state st = *stp;
  BQ_REQUIRE(st.B >= 0, BQ_EINVAL, "beam_step: bad extents");
  if (st.B == 0) return BQ_OK;
  BQ_REQUIRE(st.nb >= 1 && st.nb <= BQ_BEAM_MAX_NB && st.V >= 2 * st.nb && (long)st.nb * st.V < (1L << 31) && st.max_length >= 1 &&
                 st.max_length <= BQ_BEAM_MAX_LEN && st.Lmax >= 1 && st.Lmax <= BQ_BEAM_MAX_LEN && st.eos >= 0 && st.eos < st.V &&
                 st.pad >= 0 && st.pad < st.V && st.ld_logits >= st.V && (long)st.B * st.nb < (1L << 24),
             BQ_EINVAL, "beam_step: bad extents (B %d, nb %d, V %d, max_length %d, Lmax %d, eos %d, pad %d)", st.B, st.nb, st.V,
             st.max_length, st.Lmax, st.eos, st.pad);
  BQ_REQUIRE(st.logits && st.pos && st.lenpow && st.beam_score && st.tokens && st.anc && st.ids && st.done && st.not_done &&
                 st.src && st.cand && st.top_score && st.top_index && st.heap_len && st.heap_adds && st.heap_seq &&
                 st.heap_hyplen && st.heap_sum && st.heap_score && st.heap_worst && st.heap_tokens,
             BQ_EINVAL, "beam_step: null pointer");
  BQ_REQUIRE(((uintptr_t)st.logits & (st.logits_bf16 ? 1 : 3)) == 0, BQ_EINVAL, "beam_step: logits are not aligned to their type");
  const int S = st.B * st.nb;
  if (st.logits_bf16)
    hipLaunchKernelGGL(beam_rows_kernel<__bf16>, dim3(S), dim3(BEAM_NT), 0, (hipStream_t)stream, st);
  else
    hipLaunchKernelGGL(beam_rows_kernel<float>, dim3(S), dim3(BEAM_NT), 0, (hipStream_t)stream, st);
  hipLaunchKernelGGL(beam_sample_kernel, dim3(st.B), dim3(BEAM_NT), 0, (hipStream_t)stream, st);
  hipLaunchKernelGGL(beam_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st);
  return check_launch("beam_step");
}
