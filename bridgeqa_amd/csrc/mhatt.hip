// The attention core of MHAtt in the MCAN blocks (include/bqhip_mhatt.h states the arithmetic and its order): scores, fill,
// softmax, dropout multiplier and the product with V, forward and backward, read from and written to the (B, N, heads d) layout of
// the four linears.  bridgeqa_amd/mcan_module.py runs the same as 9 device kernels forward and 11 backward per site.
//
//   mhatt_fwd_kernel      one workgroup (4 waves) per (sample, head, TQ queries).  Pass 1: K through LDS in 64-key chunks (row
//                         pitch d + 1: a lane reading "its" key row is conflict-free), a lane per key holds the row in registers
//                         and dots it with the tile's queries (LDS broadcast); the filled logits go to an LDS row per query.
//                         Row statistics by wave max / wave sum, p stored, p keep left in LDS.  Pass 2: V through LDS in the same
//                         chunks, a lane per output column adds the keys in ascending order.
//   mhatt_bwd_q_kernel    the same tiling with (dout, V) in pass 1 (g, dp), t and ds in the middle (ds stored to the workspace),
//                         K in pass 2 (dq).
//   mhatt_bwd_kv_kernel   one wave per (sample, head, 64 keys): lane j keeps dk_j and dv_j (2 d accumulators) in registers and
//                         walks the queries in ascending order -- ds and p keep read coalesced, q_i and dout_i at wave-uniform
//                         addresses; no cross-lane reduction.  The rows leave through an LDS transpose so the stores coalesce.
//
// Two tilings of the query-major kernels, both with a 32 KB logits buffer: 32 queries x 256 keys for Nk <= 256, 8 queries x 1024
// keys beyond.  fp32, plain C++, no atomics; every sum has one order (tests/mhatt_ref.py restates it), so two runs give the same
// bits.
#include "bq_common.h"

namespace bq {

// butterfly: every level adds the same two values in both lanes of a pair, so all lanes end with the same bits
__device__ __forceinline__ float mhatt_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float mhatt_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// the workgroup copies n rows x D columns of a matrix with row stride H into LDS with row pitch D + 1
template <int D, int THREADS>
__device__ __forceinline__ void mhatt_stage(float *__restrict__ dst, const float *__restrict__ src, int n, long H, int pitch) {
  for (int idx = threadIdx.x; idx < n * D; idx += THREADS) {
    const int r = idx / D, c = idx % D;
    dst[r * pitch + c] = src[(long)r * H + c];
  }
}

// Pass 1.  row[i][j] = f(i, j, sum_c xs[i][c] y[j][c]) for the tile's nq queries and all Nk keys; query i belongs to wave i % 4.
template <int D, int TQ, int NKCAP, class F>
__device__ __forceinline__ void mhatt_dots(const float *__restrict__ y, long H, int Nk, int nq, const float *xs, float *ys,
                                           float *row, F f) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int j0 = 0; j0 < Nk; j0 += 64) {
    const int n = Nk - j0 < 64 ? Nk - j0 : 64;
    __syncthreads();   // xs is staged (first chunk); the previous chunk's readers are done
    mhatt_stage<D, 256>(ys, y + (long)j0 * H, n, H, D + 1);
    __syncthreads();
    if (lane < n) {
      float yr[D];
#pragma unroll
      for (int c = 0; c < D; ++c) yr[c] = ys[lane * (D + 1) + c];
      for (int i = wid; i < nq; i += 4) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < D; ++c) a = a + xs[i * D + c] * yr[c];
        row[i * NKCAP + j0 + lane] = f(i, j0 + lane, a);
      }
    }
  }
}

// Pass 2.  store(i, c, sum_j row[i][j] y[j][c]) for the tile's queries: the keys added in ascending order.  A wave works on
// 64 / D of its queries at once (lane = slot D + c); query i = 4 u + wave, u = pass (64 / D) + slot.
template <int D, int TQ, int NKCAP, class G>
__device__ __forceinline__ void mhatt_prod(const float *__restrict__ y, long H, int Nk, int nq, const float *row, float *ys,
                                           G store) {
  constexpr int S = 64 / D, NP = TQ / 4 / S;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane % D, slot = lane / D;
  float acc[NP];
#pragma unroll
  for (int z = 0; z < NP; ++z) acc[z] = 0.0f;
  for (int j0 = 0; j0 < Nk; j0 += 64) {
    const int n = Nk - j0 < 64 ? Nk - j0 : 64;
    __syncthreads();   // row is complete (first chunk); the previous chunk's readers are done
    mhatt_stage<D, 256>(ys, y + (long)j0 * H, n, H, D + 1);
    __syncthreads();
    for (int jj = 0; jj < n; ++jj) {
      const float yv = ys[jj * (D + 1) + c];
#pragma unroll
      for (int z = 0; z < NP; ++z) acc[z] = acc[z] + row[(4 * (z * S + slot) + wid) * NKCAP + j0 + jj] * yv;   // (rows >= nq: unused)
    }
  }
#pragma unroll
  for (int z = 0; z < NP; ++z) {
    const int i = 4 * (z * S + slot) + wid;
    if (i < nq) store(i, c, acc[z]);
  }
}

template <int D, int TQ, int NKCAP>
__global__ __launch_bounds__(256) void mhatt_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                        const float *__restrict__ v, const unsigned char *__restrict__ hide,
                                                        const float *__restrict__ keep, float *__restrict__ out,
                                                        float *__restrict__ p, int heads, int Nq, int Nk) {
  __shared__ float row[TQ * NKCAP];
  __shared__ float ys[64 * (D + 1)];
  __shared__ float xs[TQ * D];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.y / heads, h = blockIdx.y % heads, i0 = blockIdx.x * TQ;
  const int nq = Nq - i0 < TQ ? Nq - i0 : TQ;
  const long H = (long)heads * D;
  const float scale = sqrtf((float)D);
  const unsigned char *hb = hide ? hide + (long)b * Nk : nullptr;
  mhatt_stage<D, 256>(xs, q + ((long)b * Nq + i0) * H + h * D, nq, H, D);
  mhatt_dots<D, TQ, NKCAP>(k + (long)b * Nk * H + h * D, H, Nk, nq, xs, ys, row, [&](int, int j, float a) {
    const float s = a / scale;
    return (hb && hb[j]) ? -1e9f : s;
  });
  __syncthreads();
  for (int i = wid; i < nq; i += 4) {
    float *r = row + i * NKCAP;
    const long g0 = ((long)blockIdx.y * Nq + i0 + i) * Nk;
    float m = -INFINITY;
    for (int j = lane; j < Nk; j += 64) m = fmaxf(m, r[j]);
    m = mhatt_wave_max(m);
    float t = 0.0f;
    for (int j = lane; j < Nk; j += 64) {
      const float e = expf(r[j] - m);
      r[j] = e;
      t = t + e;
    }
    t = mhatt_wave_sum(t);
    for (int j = lane; j < Nk; j += 64) {
      const float pv = r[j] / t;
      p[g0 + j] = pv;
      r[j] = keep ? pv * keep[g0 + j] : pv;
    }
  }
  float *ob = out + ((long)b * Nq + i0) * H + h * D;
  mhatt_prod<D, TQ, NKCAP>(v + (long)b * Nk * H + h * D, H, Nk, nq, row, ys,
                           [&](int i, int c, float acc) { ob[(long)i * H + c] = acc; });
}

template <int D, int TQ, int NKCAP>
__global__ __launch_bounds__(256) void mhatt_bwd_q_kernel(const float *__restrict__ dout, const float *__restrict__ k,
                                                          const float *__restrict__ v, const float *__restrict__ p,
                                                          const unsigned char *__restrict__ hide, const float *__restrict__ keep,
                                                          float *__restrict__ dq, float *__restrict__ ws, int heads, int Nq,
                                                          int Nk) {
  __shared__ float row[TQ * NKCAP];
  __shared__ float ys[64 * (D + 1)];
  __shared__ float xs[TQ * D];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.y / heads, h = blockIdx.y % heads, i0 = blockIdx.x * TQ;
  const int nq = Nq - i0 < TQ ? Nq - i0 : TQ;
  const long H = (long)heads * D;
  const float scale = sqrtf((float)D);
  const unsigned char *hb = hide ? hide + (long)b * Nk : nullptr;
  const long tile0 = ((long)blockIdx.y * Nq + i0) * Nk;
  mhatt_stage<D, 256>(xs, dout + ((long)b * Nq + i0) * H + h * D, nq, H, D);
  mhatt_dots<D, TQ, NKCAP>(v + (long)b * Nk * H + h * D, H, Nk, nq, xs, ys, row,
                           [&](int i, int j, float g) { return keep ? keep[tile0 + (long)i * Nk + j] * g : g; });
  __syncthreads();
  for (int i = wid; i < nq; i += 4) {
    float *r = row + i * NKCAP;
    const long g0 = tile0 + (long)i * Nk;
    float t = 0.0f;
    for (int j = lane; j < Nk; j += 64) t = t + p[g0 + j] * r[j];
    t = mhatt_wave_sum(t);
    for (int j = lane; j < Nk; j += 64) {
      const float ds = (hb && hb[j]) ? 0.0f : p[g0 + j] * (r[j] - t);
      r[j] = ds;
      ws[g0 + j] = ds;
    }
  }
  float *ob = dq + ((long)b * Nq + i0) * H + h * D;
  mhatt_prod<D, TQ, NKCAP>(k + (long)b * Nk * H + h * D, H, Nk, nq, row, ys,
                           [&](int i, int c, float acc) { ob[(long)i * H + c] = acc / scale; });
}

template <int D>
__global__ __launch_bounds__(64) void mhatt_bwd_kv_kernel(const float *__restrict__ dout, const float *__restrict__ q,
                                                          const float *__restrict__ p, const float *__restrict__ keep,
                                                          const float *__restrict__ ws, float *__restrict__ dk,
                                                          float *__restrict__ dv, int heads, int Nq, int Nk) {
  __shared__ float tr[64 * (D + 1)];
  const int lane = threadIdx.x;
  const int b = blockIdx.y / heads, h = blockIdx.y % heads, j0 = blockIdx.x * 64;
  const int n = Nk - j0 < 64 ? Nk - j0 : 64;
  const long H = (long)heads * D;
  const float scale = sqrtf((float)D);
  const float *qb = q + (long)b * Nq * H + h * D, *db = dout + (long)b * Nq * H + h * D;
  const long col0 = (long)blockIdx.y * Nq * Nk + j0 + lane;
  float ak[D], av[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    ak[c] = 0.0f;
    av[c] = 0.0f;
  }
  for (int i = 0; i < Nq; ++i) {
    float ds = 0.0f, w = 0.0f;   // (a lane past the last key adds zeros to accumulators nobody reads)
    if (lane < n) {
      const long g = col0 + (long)i * Nk;
      ds = ws[g];
      w = keep ? p[g] * keep[g] : p[g];
    }
    const float *qi = qb + (long)i * H, *di = db + (long)i * H;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      ak[c] = ak[c] + ds * qi[c];
      av[c] = av[c] + w * di[c];
    }
  }
  float *kb = dk + ((long)b * Nk + j0) * H + h * D, *vb = dv + ((long)b * Nk + j0) * H + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) tr[lane * (D + 1) + c] = ak[c] / scale;
  __syncthreads();
  for (int idx = lane; idx < n * D; idx += 64) kb[(long)(idx / D) * H + idx % D] = tr[(idx / D) * (D + 1) + idx % D];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < D; ++c) tr[lane * (D + 1) + c] = av[c];
  __syncthreads();
  for (int idx = lane; idx < n * D; idx += 64) vb[(long)(idx / D) * H + idx % D] = tr[(idx / D) * (D + 1) + idx % D];
}

inline bool mhatt_wide(int Nk) { return Nk > 256; }   // the 8-query x 1024-key tiling

}  // namespace bq

static int mhatt_extents(const char *what, int B, int heads, int Nq, int Nk, int d) {
  using namespace bq;
  BQ_REQUIRE(B >= 0 && heads >= 1 && Nq >= 1 && Nq <= BQ_MHATT_MAX_N && Nk >= 1 && Nk <= BQ_MHATT_MAX_N && (d == 32 || d == 64),
             BQ_EINVAL, "%s: B %d, heads %d, Nq %d, Nk %d, d %d (heads >= 1, 1 <= Nq, Nk <= %d, d 32 or 64)", what, B, heads, Nq,
             Nk, d, BQ_MHATT_MAX_N);
  BQ_REQUIRE((long)B * heads <= 65535, BQ_EINVAL, "%s: B heads = %ld beyond 65535", what, (long)B * heads);
  return BQ_OK;
}

extern "C" int bqh_mhatt_fwd(const float *q, const float *k, const float *v, const unsigned char *hide, const float *keep,
                             float *out, float *p, int B, int heads, int Nq, int Nk, int d, void *stream) {
  using namespace bq;
  if (int e = mhatt_extents("mhatt_fwd", B, heads, Nq, Nk, d)) return e;
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(q && k && v && out && p, BQ_EINVAL, "mhatt_fwd: null pointer");
  with_int<32, 64>(d, [&](auto DD) {
    constexpr int D = decltype(DD)::value;
    if (mhatt_wide(Nk))
      hipLaunchKernelGGL((mhatt_fwd_kernel<D, 8, 1024>), dim3((Nq + 7) / 8, B * heads), dim3(256), 0, (hipStream_t)stream, q, k,
                         v, hide, keep, out, p, heads, Nq, Nk);
    else
      hipLaunchKernelGGL((mhatt_fwd_kernel<D, 32, 256>), dim3((Nq + 31) / 32, B * heads), dim3(256), 0, (hipStream_t)stream, q,
                         k, v, hide, keep, out, p, heads, Nq, Nk);
  });
  return check_launch("mhatt_fwd");
}

extern "C" long bqh_mhatt_bwd_ws_floats(int B, int heads, int Nq, int Nk, int d) {
  if (B <= 0 || heads < 1 || Nq < 1 || Nq > BQ_MHATT_MAX_N || Nk < 1 || Nk > BQ_MHATT_MAX_N || (d != 32 && d != 64)) return 0;
  if ((long)B * heads > 65535) return 0;
  return (long)B * heads * Nq * Nk;
}

extern "C" int bqh_mhatt_bwd(const float *dout, const float *q, const float *k, const float *v, const float *p,
                             const unsigned char *hide, const float *keep, float *dq, float *dk, float *dv, float *ws, int B,
                             int heads, int Nq, int Nk, int d, void *stream) {
  using namespace bq;
  if (int e = mhatt_extents("mhatt_bwd", B, heads, Nq, Nk, d)) return e;
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(dout && q && k && v && p && dq && dk && dv && ws, BQ_EINVAL, "mhatt_bwd: null pointer");
  with_int<32, 64>(d, [&](auto DD) {
    constexpr int D = decltype(DD)::value;
    if (mhatt_wide(Nk))
      hipLaunchKernelGGL((mhatt_bwd_q_kernel<D, 8, 1024>), dim3((Nq + 7) / 8, B * heads), dim3(256), 0, (hipStream_t)stream,
                         dout, k, v, p, hide, keep, dq, ws, heads, Nq, Nk);
    else
      hipLaunchKernelGGL((mhatt_bwd_q_kernel<D, 32, 256>), dim3((Nq + 31) / 32, B * heads), dim3(256), 0, (hipStream_t)stream,
                         dout, k, v, p, hide, keep, dq, ws, heads, Nq, Nk);
    hipLaunchKernelGGL(mhatt_bwd_kv_kernel<D>, dim3((Nk + 63) / 64, B * heads), dim3(64), 0, (hipStream_t)stream, dout, q, p,
                       keep, (const float *)ws, dk, dv, heads, Nq, Nk);
  });
  return check_launch("mhatt_bwd");
}
