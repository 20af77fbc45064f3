// Attention of answer ranking (reference models/blip_vqa_3d.py:509-566 rank_answer: k candidate answers per question are
// re-scored by the text decoder; models/med.py:179-217 BertSelfAttention.forward per layer).  N = Bq * k short sequences
// (La <= 32 tokens, BOS + answer + pad), each attending causally over itself and then over the states of ITS question --
// which the reference tiles k times and projects to K / V k times; here the K / V of a question exist once (a HoistedKV block
// with Bq rows) and sequence n reads question n / group.
//
// One WAVE per (sequence, head), four waves per workgroup; head dim 64, bf16 operands, fp32 scores / softmax / accumulation,
// bf16 output; no MFMA, no LDS, no atomics -- the layout of attn_decode.hip: lane l holds dims [8 (l & 7), +8) of a query and
// of key (l >> 3) of every group of 8 keys, a chunk of RANK_CHUNK = 32 keys is 4 such groups.  Per (query, chunk): 8 products
// per lane and key, a 3-step xor reduction over the 8 lanes of a key, s = dot * scale * log2(e) + mask (key_mask_log2 format),
// the chunk's maximum over the wave, the online-softmax rescale, p = exp2(s - m) times the lane's 8 value dims.  At the end of
// a query the 8 key groups' partial accumulators are added by a fixed xor tree that halves what a lane keeps at every step
// (8 -> 4 -> 2 -> 1 dims: 7 shuffles instead of 24), so lane l ends with output dim 8 (l & 7) + (l >> 3) and the wave stores
// the row as 64 consecutive bf16.  The tree is fixed: results are bitwise reproducible.
//
// self  : packed qkv (N, La, 3, H, 64) by strides, La <= RANK_LMAX = 32 = one chunk: the wave loads the sequence's K / V rows
//         ONCE, keeps them in registers as fp32 and walks the La queries.  Query i sees key j iff j <= i; the additive key mask
//         f32 (N, Lap) comes on top (finite values: key 0 is always in range, so every row has a finite maximum).  Pad query
//         rows are computed like any other row, as the reference computes them.
// cross : Q (N, La, H, 64), K / V (Bq, Lk, H, 64) by strides (a hoisted (Bq, Lk, 2, H, 64) block), mask f32 (Bq, Lkp); any
//         Lk >= 1 in chunks of 32 with online softmax.  The wave keeps the softmax state of RANK_QBLOCK = 4 queries in
//         registers, uses each loaded K / V chunk for all of them and loops over query blocks.
// Keys beyond the count are never loaded; their registers are zero and their probability is exactly 0.
#include "bq_common.h"

namespace bq {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int RANK_CHUNK = 32;   // keys per online-softmax step = 4 groups of 8 keys
constexpr int RANK_LMAX = 32;    // self form: the whole sequence is one chunk (BQ_RANK_LMAX)
constexpr int RANK_QBLOCK = 4;   // cross form: queries whose softmax state a wave holds at once (BQ_RANK_QBLOCK)
constexpr int RANK_WAVES = 4;
static_assert(RANK_LMAX == BQ_RANK_LMAX && RANK_QBLOCK == BQ_RANK_QBLOCK, "bqhip_fusion.h");

__device__ __forceinline__ bf16x8 rk_load8(const __bf16 *p) { return *reinterpret_cast<const bf16x8 *>(p); }

__device__ __forceinline__ void rk_unpack(const bf16x8 x, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (float)x[e];
}

// keys base + 8 i + grp (i < 4) of one (row block, head): fp32 K / V dims [dc, dc + 8) and the mask value; zero beyond n
__device__ __forceinline__ void rk_load_chunk(const __bf16 *K, const __bf16 *V, const float *mask_row, int base, int n, int grp,
                                              long k_rs, float (&kf)[4][8], float (&vf)[4][8], float (&mk)[4]) {
  bf16x8 kk[4], vv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = base + 8 * i + grp;
#pragma unroll
    for (int e = 0; e < 8; ++e) kk[i][e] = vv[i][e] = (__bf16)0.f;
    mk[i] = 0.f;
    if (j < n) {
      kk[i] = rk_load8(K + j * k_rs);
      vv[i] = rk_load8(V + j * k_rs);
      if (mask_row != nullptr) mk[i] = mask_row[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rk_unpack(kk[i], kf[i]);
    rk_unpack(vv[i], vf[i]);
  }
}

// one query against one chunk: lim = number of keys of the chunk's range [base, ...) this query may see (absolute index)
__device__ __forceinline__ void rk_step(const float (&q)[8], const float (&kf)[4][8], const float (&vf)[4][8], const float (&mk)[4],
                                        int base, int lim, int grp, float scale_log2, float &m, float &l, float (&acc)[8]) {
  float sc[4];
  float cmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) d = fmaf(q[e], kf[i][e], d);
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 4);
    sc[i] = base + 8 * i + grp < lim ? d * scale_log2 + mk[i] : -INFINITY;
    cmax = fmaxf(cmax, sc[i]);
  }
  cmax = fmaxf(cmax, __shfl_xor(cmax, 8));
  cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
  cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
  const float mn = fmaxf(m, cmax);  // finite: every chunk a query meets holds at least one key it sees
  const float alpha = __builtin_amdgcn_exp2f(m - mn);
  l *= alpha;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float p = __builtin_amdgcn_exp2f(sc[i] - mn);  // exp2(-inf) = 0 for a key out of range; its V registers are 0
    l += p;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, vf[i][e], acc[e]);
  }
  m = mn;
}

// the 8 key groups' partial states share m.  l: a plain xor tree.  acc: at every step a lane hands the half it drops to its
// partner and adds the partner's half of what it keeps; lane (grp, c) ends with dim 8 c + grp of the row.
__device__ __forceinline__ void rk_finish(float l, const float (&acc)[8], int lane, __bf16 *o_row) {
  l += __shfl_xor(l, 8);
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const bool b32 = (lane & 32) != 0, b16 = (lane & 16) != 0, b8 = (lane & 8) != 0;
  float a4[4], a2[2];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float keep = b32 ? acc[e + 4] : acc[e], give = b32 ? acc[e] : acc[e + 4];
    a4[e] = keep + __shfl_xor(give, 32);
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float keep = b16 ? a4[e + 2] : a4[e], give = b16 ? a4[e] : a4[e + 2];
    a2[e] = keep + __shfl_xor(give, 16);
  }
  const float keep = b8 ? a2[1] : a2[0], give = b8 ? a2[0] : a2[1];
  const float a = keep + __shfl_xor(give, 8);
  o_row[(lane & 7) * 8 + (lane >> 3)] = (__bf16)(a * (1.0f / l));
}

__global__ __launch_bounds__(64 * RANK_WAVES) void attn_rank_self_kernel(
    const __bf16 *__restrict__ QKV, __bf16 *__restrict__ O, const float *__restrict__ mask, int N, int H, int La, int Lap,
    long q_bs, long q_rs, long q_ks, long q_hs, long o_bs, long o_rs, long o_hs, float scale_log2) {
  const int w = blockIdx.x * RANK_WAVES + (threadIdx.x >> 6);
  if (w >= N * H) return;  // wave-uniform
  const int n = w / H, h = w % H;
  const int lane = threadIdx.x & 63, grp = lane >> 3, dc = (lane & 7) * 8;
  const __bf16 *qp = QKV + n * q_bs + h * q_hs + dc;
  float kf[4][8], vf[4][8], mk[4];
  rk_load_chunk(qp + q_ks, qp + 2 * q_ks, mask != nullptr ? mask + (long)n * Lap : nullptr, 0, La, grp, q_rs, kf, vf, mk);
  __bf16 *op = O + n * o_bs + h * o_hs;
  for (int i = 0; i < La; ++i) {
    float q[8], acc[8], m = -INFINITY, l = 0.f;
    rk_unpack(rk_load8(qp + i * q_rs), q);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    rk_step(q, kf, vf, mk, 0, i + 1, grp, scale_log2, m, l, acc);  // causal: keys 0 .. i
    rk_finish(l, acc, lane, op + i * o_rs);
  }
}

__global__ __launch_bounds__(64 * RANK_WAVES) void attn_rank_cross_kernel(
    const __bf16 *__restrict__ Q, const __bf16 *__restrict__ K, const __bf16 *__restrict__ V, __bf16 *__restrict__ O,
    const float *__restrict__ mask, int N, int H, int La, int Lk, int Lkp, int group, long q_bs, long q_rs, long q_hs, long k_bs,
    long k_rs, long k_hs, long o_bs, long o_rs, long o_hs, float scale_log2) {
  const int w = blockIdx.x * RANK_WAVES + (threadIdx.x >> 6);
  if (w >= N * H) return;  // wave-uniform
  const int n = w / H, h = w % H, b = n / group;
  const int lane = threadIdx.x & 63, grp = lane >> 3, dc = (lane & 7) * 8;
  const __bf16 *qp = Q + n * q_bs + h * q_hs + dc;
  const long koff = b * k_bs + h * k_hs + dc;
  const float *mrow = mask != nullptr ? mask + (long)b * Lkp : nullptr;
  __bf16 *op = O + n * o_bs + h * o_hs;
  for (int i0 = 0; i0 < La; i0 += RANK_QBLOCK) {
    float q[RANK_QBLOCK][8], acc[RANK_QBLOCK][8], m[RANK_QBLOCK], l[RANK_QBLOCK];
#pragma unroll
    for (int r = 0; r < RANK_QBLOCK; ++r) {
      m[r] = -INFINITY;
      l[r] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) q[r][e] = acc[r][e] = 0.f;
      if (i0 + r < La) rk_unpack(rk_load8(qp + (i0 + r) * q_rs), q[r]);  // wave-uniform
    }
    for (int base = 0; base < Lk; base += RANK_CHUNK) {
      float kf[4][8], vf[4][8], mk[4];
      rk_load_chunk(K + koff, V + koff, mrow, base, Lk, grp, k_rs, kf, vf, mk);
#pragma unroll
      for (int r = 0; r < RANK_QBLOCK; ++r)
        if (i0 + r < La) rk_step(q[r], kf, vf, mk, base, Lk, grp, scale_log2, m[r], l[r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RANK_QBLOCK; ++r)
      if (i0 + r < La) rk_finish(l[r], acc[r], lane, op + (i0 + r) * o_rs);
  }
}

static bool rk_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static bool rk_mult8(long a, long b = 0, long c = 0, long d = 0) { return ((a | b | c | d) & 7) == 0; }

}  // namespace bq

extern "C" int bq_attn_rank_self(const void *qkv, void *O, const float *mask, int N, int H, int La, int Lap, long q_bs, long q_rs,
                                 long q_ks, long q_hs, long o_bs, long o_rs, long o_hs, float scale, void *stream) {
  using namespace bq;
  BQ_REQUIRE(N >= 0, BQ_EINVAL, "attn_rank_self: bad extents");
  if (N == 0) return BQ_OK;
  BQ_REQUIRE(qkv && O && H > 0 && La > 0 && (!mask || Lap >= La), BQ_EINVAL, "attn_rank_self: null pointer or bad extents");
  BQ_REQUIRE(La <= RANK_LMAX, BQ_ELIMIT, "attn_rank_self: %d tokens per sequence, the kernel holds %d", La, RANK_LMAX);
  BQ_REQUIRE(rk_aligned16(qkv) && rk_aligned16(O) && rk_mult8(q_bs, q_rs, q_ks, q_hs) && rk_mult8(o_bs, o_rs, o_hs), BQ_EINVAL,
             "attn_rank_self: operands must be 16-byte aligned with strides in multiples of 8");
  BQ_REQUIRE((long)N * H < (1L << 31) - RANK_WAVES, BQ_ELIMIT, "attn_rank_self: too many (sequence, head) items");
  hipLaunchKernelGGL(attn_rank_self_kernel, dim3((unsigned)(((long)N * H + RANK_WAVES - 1) / RANK_WAVES)), dim3(64 * RANK_WAVES), 0,
                     (hipStream_t)stream, (const __bf16 *)qkv, (__bf16 *)O, mask, N, H, La, Lap, q_bs, q_rs, q_ks, q_hs, o_bs,
                     o_rs, o_hs, scale * 1.4426950408889634f);
  return check_launch("attn_rank_self");
}

extern "C" int bq_attn_rank_cross(const void *Q, const void *K, const void *V, void *O, const float *mask, int N, int Bq, int group,
                                  int H, int La, int Lk, int Lkp, long q_bs, long q_rs, long q_hs, long k_bs, long k_rs,
                                  long k_hs, long o_bs, long o_rs, long o_hs, float scale, void *stream) {
  using namespace bq;
  BQ_REQUIRE(N >= 0, BQ_EINVAL, "attn_rank_cross: bad extents");
  if (N == 0) return BQ_OK;
  BQ_REQUIRE(Q && K && V && O && H > 0 && La > 0 && Lk > 0 && (!mask || Lkp >= Lk), BQ_EINVAL,
             "attn_rank_cross: null pointer or bad extents");
  BQ_REQUIRE(group > 0 && Bq > 0 && (long)Bq * group == N, BQ_EINVAL,
             "attn_rank_cross: %d sequences are not %d questions x %d candidates", N, Bq, group);
  BQ_REQUIRE(rk_aligned16(Q) && rk_aligned16(K) && rk_aligned16(V) && rk_aligned16(O) && rk_mult8(q_bs, q_rs, q_hs) &&
                 rk_mult8(k_bs, k_rs, k_hs) && rk_mult8(o_bs, o_rs, o_hs), BQ_EINVAL,
             "attn_rank_cross: operands must be 16-byte aligned with strides in multiples of 8");
  BQ_REQUIRE((long)N * H < (1L << 31) - RANK_WAVES, BQ_ELIMIT, "attn_rank_cross: too many (sequence, head) items");
  hipLaunchKernelGGL(attn_rank_cross_kernel, dim3((unsigned)(((long)N * H + RANK_WAVES - 1) / RANK_WAVES)), dim3(64 * RANK_WAVES), 0,
                     (hipStream_t)stream, (const __bf16 *)Q, (const __bf16 *)K, (const __bf16 *)V, (__bf16 *)O, mask, N, H, La,
                     Lk, Lkp, group, q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, o_bs, o_rs, o_hs, scale * 1.4426950408889634f);
  return check_launch("attn_rank_cross");
}
