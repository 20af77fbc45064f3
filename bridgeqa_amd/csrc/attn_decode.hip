// Single-query attention for beam-search decoding (reference models/med.py:179-217 BertSelfAttention.forward with
// past_key_value set, as HF's GenerationMixin drives it from the second token on: one new token per beam slot attends over
// the cached keys / values of its hypothesis, then over the question states).
//
// One WAVE per (slot, head), four waves per workgroup; head dim 64, bf16 operands, fp32 scores / softmax / accumulation,
// bf16 output.  A latency and bandwidth kernel: no MFMA, no LDS -- K / V rows go straight to registers with 16-byte loads.
// Lane l holds dims [8 (l & 7), +8) of the query and of key (l >> 3) of every group of 8 keys; a chunk of DEC_CHUNK = 32
// keys is 4 such groups, all 8 loads of a lane in flight together.  Per chunk: 8 products per lane, a 3-step xor reduction
// over the 8 lanes of a key, s = dot * scale * log2(e) + mask (key_mask_log2 format, as bq_attn_fwd), the chunk's maximum over
// the wave, the online-softmax rescale and p = exp2(s - m) times the lane's 8 value dims.  The 8 key groups' partial sums
// and accumulators are added by xor shuffles at the end (a fixed tree: deterministic, no atomics).
//
// self  : the step's packed projection qkv (S, 1, 3, H, 64) and the layer's STATIC cache KV (S, Lmax, 2, H, 64).  The wave
//         of (s, h) stores its own K / V row into KV[s, t] and attends over positions 0..t: position j < t of slot s is cache
//         row anc[j][s] (the beam ancestry: beam search reorders hypotheses, the cache stays in place), position t comes from
//         the wave's registers -- it is not re-read, so no wave depends on another's store within the launch (other waves
//         only read positions < t).  t is read from a device pointer so that a captured step can be replayed.
// cross : K / V by strides (a HoistedKV block (S, Lk, 2, H, 64)), additive key mask f32 (S, Lkp) times log2(e); no ancestry:
//         the question states belong to the beam SLOT (generation.py docstring).
// Keys beyond the count are never loaded (a cache holds garbage there), out-of-range ancestry rows / positions are clamped
// into the cache: a wrong table gives a wrong answer, never an access outside the buffers.
#include "bq_common.h"

namespace bq {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int DEC_CHUNK = 32;  // keys per online-softmax step = 4 groups of 8 keys (tests/test_attn_decode_gpu.py walks its edges)
constexpr int DEC_WAVES = 4;

__device__ __forceinline__ bf16x8 load8(const __bf16 *p) { return *reinterpret_cast<const bf16x8 *>(p); }

template <bool SELF>
__global__ __launch_bounds__(64 * DEC_WAVES) void attn_decode_kernel(
    const __bf16 *__restrict__ Q, const __bf16 *K, const __bf16 *V, __bf16 *__restrict__ O, const float *__restrict__ mask,
    const int *__restrict__ anc, const int *__restrict__ t_ptr, int t_host, __bf16 *cache, int S, int H, int Lk, int Lmax,
    int Lkp, long q_bs, long q_ks, long q_hs, long k_bs, long k_rs, long k_hs, long o_bs, long o_hs, float scale_log2) {
  const int w = blockIdx.x * DEC_WAVES + (threadIdx.x >> 6);
  if (w >= S * H) return;  // wave-uniform
  const int s = w / H, h = w % H;
  const int lane = threadIdx.x & 63, grp = lane >> 3, dc = (lane & 7) * 8;
  int t = 0;
  if (SELF) {
    t = t_ptr ? *t_ptr : t_host;
    t = min(max(t, 0), Lmax - 1);
  }
  const int n = SELF ? t + 1 : Lk;

  const __bf16 *qp = Q + s * q_bs + h * q_hs + dc;
  float q[8];
  {
    const bf16x8 x = load8(qp);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = (float)x[e];
  }
  bf16x8 knew, vnew;
#pragma unroll
  for (int e = 0; e < 8; ++e) knew[e] = vnew[e] = (__bf16)0.f;
  if (SELF) {
    knew = load8(qp + q_ks);
    vnew = load8(qp + 2 * q_ks);
    if (grp == 0) {  // the row of this step: KV[s, t, 0 / 1, h, :]
      __bf16 *cp = cache + s * k_bs + t * k_rs + h * k_hs + dc;
      *reinterpret_cast<bf16x8 *>(cp) = knew;
      *reinterpret_cast<bf16x8 *>(cp + (V - K)) = vnew;
    }
  }

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;

  for (int base = 0; base < n; base += DEC_CHUNK) {
    bf16x8 kk[4], vv[4];
    float sc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = base + 8 * i + grp;
      kk[i] = knew;  // j == t (self); overwritten or unused otherwise
      vv[i] = vnew;
      if (SELF ? j < t : j < n) {
        long row = s;
        if (SELF) row = min(max(anc[(long)j * S + s], 0), S - 1);
        const long off = row * k_bs + j * k_rs + h * k_hs + dc;
        kk[i] = load8(K + off);
        vv[i] = load8(V + off);
      }
    }
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = base + 8 * i + grp;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(q[e], (float)kk[i][e], d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      float x = d * scale_log2;
      if (!SELF && mask != nullptr && j < n) x += mask[(long)s * Lkp + j];
      sc[i] = j < n ? x : -INFINITY;
      cmax = fmaxf(cmax, sc[i]);
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 8));
    cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
    const float mn = fmaxf(m, cmax);  // finite: every chunk holds at least one key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = base + 8 * i + grp;
      if (j < n) {  // (a key beyond the count holds no loaded value: its registers are not multiplied at all)
        const float p = __builtin_amdgcn_exp2f(sc[i] - mn);
        l += p;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, (float)vv[i][e], acc[e]);
      }
    }
    m = mn;
  }
  // the 8 key groups' partial states share m: add them in a fixed xor tree
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    l += __shfl_xor(l, off);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], off);
  }
  if (grp == 0) {
    const float inv = 1.0f / l;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)(acc[e] * inv);
    *reinterpret_cast<bf16x8 *>(O + s * o_bs + h * o_hs + dc) = o;
  }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static bool mult8(long a, long b = 0, long c = 0, long d = 0) { return ((a | b | c | d) & 7) == 0; }

}  // namespace bq

extern "C" int bq_attn_decode_self(const void *qkv, void *kv_cache, const int32_t *anc, void *O, const int *t_ptr, int t,
                                   int S, int H, int Lmax, long q_bs, long q_ks, long q_hs, long c_bs, long c_rs, long c_ks,
                                   long c_hs, long o_bs, long o_hs, float scale, void *stream) {
  using namespace bq;
  BQ_REQUIRE(S >= 0, BQ_EINVAL, "attn_decode_self: bad extents");
  if (S == 0) return BQ_OK;
  BQ_REQUIRE(qkv && kv_cache && anc && O && H > 0 && Lmax > 0, BQ_EINVAL, "attn_decode_self: null pointer or bad extents");
  BQ_REQUIRE(t_ptr || (t >= 0 && t < Lmax), BQ_EINVAL, "attn_decode_self: position %d outside the cache (Lmax %d)", t, Lmax);
  BQ_REQUIRE(aligned16(qkv) && aligned16(kv_cache) && aligned16(O) && mult8(q_bs, q_ks, q_hs) && mult8(c_bs, c_rs, c_ks, c_hs) &&
                 mult8(o_bs, o_hs), BQ_EINVAL, "attn_decode_self: operands must be 16-byte aligned with strides in multiples of 8");
  BQ_REQUIRE((long)S * H < (1L << 31) - DEC_WAVES, BQ_ELIMIT, "attn_decode_self: too many (slot, head) items");
  __bf16 *c = (__bf16 *)kv_cache;
  hipLaunchKernelGGL(attn_decode_kernel<true>, dim3((unsigned)(((long)S * H + DEC_WAVES - 1) / DEC_WAVES)), dim3(64 * DEC_WAVES),
                     0, (hipStream_t)stream, (const __bf16 *)qkv, c, c + c_ks, (__bf16 *)O, (const float *)nullptr, anc, t_ptr, t,
                     c, S, H, 0, Lmax, 0, q_bs, q_ks, q_hs, c_bs, c_rs, c_hs, o_bs, o_hs, scale * 1.4426950408889634f);
  return check_launch("attn_decode_self");
}

extern "C" int bq_attn_decode_cross(const void *Q, const void *K, const void *V, void *O, const float *mask, int S, int H,
                                    int Lk, int Lkp, long q_bs, long q_hs, long k_bs, long k_rs, long k_hs, long o_bs,
                                    long o_hs, float scale, void *stream) {
  using namespace bq;
  BQ_REQUIRE(S >= 0, BQ_EINVAL, "attn_decode_cross: bad extents");
  if (S == 0) return BQ_OK;
  BQ_REQUIRE(Q && K && V && O && H > 0 && Lk > 0 && (!mask || Lkp >= Lk), BQ_EINVAL,
             "attn_decode_cross: null pointer or bad extents");
  BQ_REQUIRE(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(O) && mult8(q_bs, q_hs) && mult8(k_bs, k_rs, k_hs) &&
                 mult8(o_bs, o_hs), BQ_EINVAL, "attn_decode_cross: operands must be 16-byte aligned with strides in multiples of 8");
  BQ_REQUIRE((long)S * H < (1L << 31) - DEC_WAVES, BQ_ELIMIT, "attn_decode_cross: too many (slot, head) items");
  hipLaunchKernelGGL(attn_decode_kernel<false>, dim3((unsigned)(((long)S * H + DEC_WAVES - 1) / DEC_WAVES)), dim3(64 * DEC_WAVES),
                     0, (hipStream_t)stream, (const __bf16 *)Q, (const __bf16 *)K, (const __bf16 *)V, (__bf16 *)O, mask,
                     (const int *)nullptr, (const int *)nullptr, 0, (__bf16 *)nullptr, S, H, Lk, 0, Lkp, q_bs, 0L, q_hs, k_bs, k_rs,
                     k_hs, o_bs, o_hs, scale * 1.4426950408889634f);
  return check_launch("attn_decode_cross");
}
