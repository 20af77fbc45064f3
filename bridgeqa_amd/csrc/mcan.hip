// The row operators of the MCAN blocks (include/bqhip_mcan.h states the arithmetic and its order): MCAN's residual LayerNorm
// -- a_2 (z - mean) / (sigma_unbiased + eps) + b_2 over z = x + s, which csrc/ln.hip's rsqrt(var + eps) cannot serve -- and
// AttFlat's masked softmax pooling, forward and backward.  bridgeqa_amd/mcan_module.py runs them as ~11 and ~8 torch launches.
//
//   mcan_ln_fwd_kernel     one wave per row, a lane holds H / 64 values (columns i 64 + lane), statistics by wave sums
//   mcan_ln_bwd_kernel     rows strided over the grid; every wave folds its rows' da2 / db2 in registers, one LDS fold over the
//                          4 waves, the workgroup's partial row STORED to a slab
//   mcan_ln_fold_kernel    adds the slab's rows in a fixed tree order
//   mcan_pool_fwd_kernel   one wave per (sample, 64 columns): softmax of the sample's logits into LDS, then the weighted sum
//                          over the keys in ascending order
//   mcan_pool_bwd_kernel   one workgroup per sample: dx and da (in LDS) by one wave per key, then t and dlogits by one wave per
//                          glimpse
//
// fp32, plain C++, no atomics; every sum has one order (tests/mcan_ref.py restates it), so two runs give the same bits.
#include "bq_common.h"

namespace bq {

// butterfly: every level adds the same two values in both lanes of a pair, so all lanes end with the same bits
__device__ __forceinline__ float mcan_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float mcan_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

template <int NV>
__global__ __launch_bounds__(256) void mcan_ln_fwd_kernel(const float *__restrict__ x, const float *__restrict__ s,
                                                          const float *__restrict__ a2, const float *__restrict__ b2,
                                                          float *__restrict__ y, float *__restrict__ mean_out,
                                                          float *__restrict__ sigma_out, int M, float eps) {
  constexpr int H = NV * 64;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const long off = (long)row * H + lane;
  float z[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) z[i] = x[off + i * 64];
  if (s) {
#pragma unroll
    for (int i = 0; i < NV; ++i) z[i] = z[i] + s[off + i * 64];
  }
  float t = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) t = t + z[i];
  const float mean = mcan_wave_sum(t) / (float)H;
  float v = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    z[i] = z[i] - mean;
    v = v + z[i] * z[i];
  }
  const float sigma = sqrtf(mcan_wave_sum(v) / (float)(H - 1));
  const float r = 1.0f / (sigma + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) y[off + i * 64] = a2[i * 64 + lane] * (z[i] * r) + b2[i * 64 + lane];
  if (lane == 0) {
    mean_out[row] = mean;
    sigma_out[row] = sigma;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void mcan_ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                          const float *__restrict__ s, const float *__restrict__ a2,
                                                          const float *__restrict__ mean_in, const float *__restrict__ sigma_in,
                                                          float *__restrict__ dz, float *__restrict__ slab, int M, float eps) {
  constexpr int H = NV * 64;
  __shared__ float red[4][2 * H];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float w[NV], acc_a[NV], acc_b[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    w[i] = a2[i * 64 + lane];
    acc_a[i] = 0.0f;
    acc_b[i] = 0.0f;
  }
  for (int row = blockIdx.x * 4 + wid; row < M; row += gridDim.x * 4) {
    const long off = (long)row * H + lane;
    const float mean = mean_in[row], sigma = sigma_in[row];
    const float r = 1.0f / (sigma + eps);
    const float k = (r * r) / ((float)(H - 1) * sigma);
    float c[NV], g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) c[i] = x[off + i * 64];
    if (s) {
#pragma unroll
      for (int i = 0; i < NV; ++i) c[i] = c[i] + s[off + i * 64];
    }
    float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const float d = dy[off + i * 64];
      c[i] = c[i] - mean;
      g[i] = d * w[i];
      t1 = t1 + g[i];
      t2 = t2 + g[i] * c[i];
      acc_a[i] = acc_a[i] + d * (c[i] * r);
      acc_b[i] = acc_b[i] + d;
    }
    const float s1 = mcan_wave_sum(t1) / (float)H;
    const float ks2 = k * mcan_wave_sum(t2);
#pragma unroll
    for (int i = 0; i < NV; ++i) dz[off + i * 64] = r * (g[i] - s1) - ks2 * c[i];
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    red[wid][i * 64 + lane] = acc_a[i];
    red[wid][H + i * 64 + lane] = acc_b[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * H; c += 256)
    slab[(long)blockIdx.x * (2 * H) + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// out[c] = the sum of the `rows` rows of slab (rows, W) in a fixed order that is a tree, not a chain (rows <= 256: a chain of
// partials errs like a sum of 256 terms, this like one of 13): 64 columns x 4 row phases per workgroup, a thread's 8 accumulators
// take rows ph + 4 u + 32 i for ascending i, then ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) and (p0 + p1) + (p2 + p3)
__global__ __launch_bounds__(256) void mcan_ln_fold_kernel(const float *__restrict__ slab, float *__restrict__ out, int rows,
                                                           int W) {
  __shared__ float sm[4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float t[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) t[u] = 0.0f;
  if (c < W) {
    for (int base = ph; base < rows; base += 32) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (base + 4 * u < rows) t[u] = t[u] + slab[(long)(base + 4 * u) * W + c];
    }
  }
  sm[ph][cl] = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  __syncthreads();
  if (ph == 0 && c < W) out[c] = (sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl]);
}

__global__ __launch_bounds__(64) void mcan_pool_fwd_kernel(const float *__restrict__ x, const float *__restrict__ logits,
                                                           const unsigned char *__restrict__ hide, float *__restrict__ out,
                                                           float *__restrict__ p_out, int N, int G, int H) {
  __shared__ float ps[BQ_MCAN_MAX_G][BQ_MCAN_MAX_N];
  const int lane = threadIdx.x, b = blockIdx.y;
  const long row0 = (long)b * N;
  for (int g = 0; g < G; ++g) {
    float m = -INFINITY;
    for (int n = lane; n < N; n += 64) {
      const float l = (hide && hide[row0 + n]) ? -1e9f : logits[(row0 + n) * G + g];
      ps[g][n] = l;
      m = fmaxf(m, l);
    }
    m = mcan_wave_max(m);
    float t = 0.0f;
    for (int n = lane; n < N; n += 64) {
      const float e = expf(ps[g][n] - m);
      ps[g][n] = e;
      t = t + e;
    }
    t = mcan_wave_sum(t);
    for (int n = lane; n < N; n += 64) {
      const float p = ps[g][n] / t;
      ps[g][n] = p;
      if (blockIdx.x == 0) p_out[(row0 + n) * G + g] = p;
    }
  }
  __syncthreads();
  const int h = blockIdx.x * 64 + lane;
  const float *xc = x + row0 * H + h;
  float acc[BQ_MCAN_MAX_G] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
  for (int n = 0; n < N; ++n) {
    const float xv = xc[(long)n * H];
#pragma unroll
    for (int g = 0; g < BQ_MCAN_MAX_G; ++g)
      if (g < G) acc[g] = acc[g] + ps[g][n] * xv;
  }
#pragma unroll
  for (int g = 0; g < BQ_MCAN_MAX_G; ++g)
    if (g < G) out[((long)b * G + g) * H + h] = acc[g];
}

__global__ __launch_bounds__(256) void mcan_pool_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ x,
                                                            const float *__restrict__ p, const unsigned char *__restrict__ hide,
                                                            float *__restrict__ dx, float *__restrict__ dlogits, int N, int G,
                                                            int H) {
  __shared__ float ds[BQ_MCAN_MAX_G][BQ_MCAN_MAX_H];
  __shared__ float da[BQ_MCAN_MAX_G][BQ_MCAN_MAX_N];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, b = blockIdx.x;
  const long row0 = (long)b * N;
  for (int i = threadIdx.x; i < G * H; i += 256) ds[i / H][i % H] = dout[(long)b * G * H + i];
  __syncthreads();
  for (int n = wid; n < N; n += 4) {
    float pg[BQ_MCAN_MAX_G], acc[BQ_MCAN_MAX_G];
#pragma unroll
    for (int g = 0; g < BQ_MCAN_MAX_G; ++g) {
      pg[g] = g < G ? p[(row0 + n) * G + g] : 0.0f;
      acc[g] = 0.0f;
    }
    for (int h = lane; h < H; h += 64) {
      const float xv = x[(row0 + n) * H + h];
      float d = pg[0] * ds[0][h];
      acc[0] = acc[0] + xv * ds[0][h];
#pragma unroll
      for (int g = 1; g < BQ_MCAN_MAX_G; ++g)
        if (g < G) {
          d = d + pg[g] * ds[g][h];
          acc[g] = acc[g] + xv * ds[g][h];
        }
      dx[(row0 + n) * H + h] = d;
    }
#pragma unroll
    for (int g = 0; g < BQ_MCAN_MAX_G; ++g)
      if (g < G) {
        const float a = mcan_wave_sum(acc[g]);
        if (lane == 0) da[g][n] = a;
      }
  }
  __syncthreads();
  if (wid < G) {
    const int g = wid;
    float t = 0.0f;
    for (int n = lane; n < N; n += 64) t = t + p[(row0 + n) * G + g] * da[g][n];
    t = mcan_wave_sum(t);
    for (int n = lane; n < N; n += 64) {
      const float pv = p[(row0 + n) * G + g];
      dlogits[(row0 + n) * G + g] = (hide && hide[row0 + n]) ? 0.0f : pv * (da[g][n] - t);
    }
  }
}

inline bool mcan_h_ok(int H) { return H >= 64 && H <= BQ_MCAN_MAX_H && H % 64 == 0; }
inline int mcan_ln_bwd_blocks(int M) {
  const int b = (M + 3) / 4;
  return b < BQ_MCAN_LN_BWD_CAP ? b : BQ_MCAN_LN_BWD_CAP;
}

}  // namespace bq

extern "C" int bqm_mcan_ln_fwd(const float *x, const float *s, const float *a2, const float *b2, float *y, float *mean,
                               float *sigma, int M, int H, float eps, void *stream) {
  using namespace bq;
  BQ_REQUIRE(M >= 0 && mcan_h_ok(H), BQ_EINVAL, "mcan_ln_fwd: M %d, H %d (H: a multiple of 64 in [64, %d])", M, H, BQ_MCAN_MAX_H);
  if (M == 0) return BQ_OK;
  BQ_REQUIRE(x && a2 && b2 && y && mean && sigma, BQ_EINVAL, "mcan_ln_fwd: null pointer");
  with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(H / 64, [&](auto NV) {
    hipLaunchKernelGGL(mcan_ln_fwd_kernel<decltype(NV)::value>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, s, a2,
                       b2, y, mean, sigma, M, eps);
  });
  return check_launch("mcan_ln_fwd");
}

extern "C" long bqm_mcan_ln_bwd_slab_floats(int M, int H) {
  using namespace bq;
  if (M <= 0 || !mcan_h_ok(H)) return 0;
  return (long)mcan_ln_bwd_blocks(M) * 2 * H;
}

extern "C" int bqm_mcan_ln_bwd(const float *dy, const float *x, const float *s, const float *a2, const float *mean,
                               const float *sigma, float *dz, float *dab, float *slab, int M, int H, float eps, void *stream) {
  using namespace bq;
  BQ_REQUIRE(M >= 1 && mcan_h_ok(H), BQ_EINVAL, "mcan_ln_bwd: M %d, H %d (M >= 1; H: a multiple of 64 in [64, %d])", M, H,
             BQ_MCAN_MAX_H);
  BQ_REQUIRE(dy && x && a2 && mean && sigma && dz && dab && slab, BQ_EINVAL, "mcan_ln_bwd: null pointer");
  const int blocks = mcan_ln_bwd_blocks(M);
  with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(H / 64, [&](auto NV) {
    hipLaunchKernelGGL(mcan_ln_bwd_kernel<decltype(NV)::value>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, x, s, a2,
                       mean, sigma, dz, slab, M, eps);
  });
  hipLaunchKernelGGL(mcan_ln_fold_kernel, dim3((2 * H + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float *)slab, dab,
                     blocks, 2 * H);
  return check_launch("mcan_ln_bwd");
}

static int mcan_pool_extents(const char *what, int B, int N, int G, int H) {
  using namespace bq;
  BQ_REQUIRE(B >= 0 && N >= 1 && N <= BQ_MCAN_MAX_N && G >= 1 && G <= BQ_MCAN_MAX_G && mcan_h_ok(H), BQ_EINVAL,
             "%s: B %d, N %d, G %d, H %d (1 <= N <= %d, 1 <= G <= %d, H: a multiple of 64 up to %d)", what, B, N, G, H,
             BQ_MCAN_MAX_N, BQ_MCAN_MAX_G, BQ_MCAN_MAX_H);
  BQ_REQUIRE(B <= 65535, BQ_EINVAL, "%s: B %d beyond 65535", what, B);
  return BQ_OK;
}

extern "C" int bqm_attflat_pool_fwd(const float *x, const float *logits, const unsigned char *hide, float *out, float *p, int B,
                                    int N, int G, int H, void *stream) {
  using namespace bq;
  if (int e = mcan_pool_extents("attflat_pool_fwd", B, N, G, H)) return e;
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(x && logits && out && p, BQ_EINVAL, "attflat_pool_fwd: null pointer");
  hipLaunchKernelGGL(mcan_pool_fwd_kernel, dim3(H / 64, B), dim3(64), 0, (hipStream_t)stream, x, logits, hide, out, p, N, G, H);
  return check_launch("attflat_pool_fwd");
}

extern "C" int bqm_attflat_pool_bwd(const float *dout, const float *x, const float *p, const unsigned char *hide, float *dx,
                                    float *dlogits, int B, int N, int G, int H, void *stream) {
  using namespace bq;
  if (int e = mcan_pool_extents("attflat_pool_bwd", B, N, G, H)) return e;
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(dout && x && p && dx && dlogits, BQ_EINVAL, "attflat_pool_bwd: null pointer");
  hipLaunchKernelGGL(mcan_pool_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dout, x, p, hide, dx, dlogits, N, G, H);
  return check_launch("attflat_pool_bwd");
}
