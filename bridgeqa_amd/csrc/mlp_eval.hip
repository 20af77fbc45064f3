// Eval-mode SharedMLP of one detector module in ONE launch (bq_mlp_eval, include/bqhip_fusion.h): up to three
// 1x1 convolution -> BatchNorm(eval) -> ReLU layers (+ max over nsample, or + one fp32 linear tail), bf16 operands on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  Eval-mode BatchNorm is the fixed per-channel map y = acc s + t,
// s = gamma rsqrt(running_var + eps), t = beta + (bias - running_mean) s, formed in every workgroup's prologue from the live
// parameters and buffers (nothing cached on the host).
//
// A workgroup (4 waves) owns ME_TM = 64 rows.  Its input rows go to LDS once -- gathered from the point-major fp32 features
// by the ball-query index (the grouped form: the same bf16 values csrc/pn2_ops.hip group_concat_pm writes; the grouped
// tensor is never written) or copied from bf16 rows (the rows form).  Each layer reads its activation tile from LDS and
// writes its bf16-rounded output tile to the other LDS buffer: no intermediate activation reaches HBM.
// Orientation: D^T = W X^T, A = weight rows (16 output channels x 32 k, one 16-byte global load per lane, L2-resident, the
// next k-step's fragments in flight under the current MFMAs), B = activation rows (one ds_read_b128 per lane and 16-row
// block), so a lane's four accumulators are four CONSECUTIVE channels of one row: one 8-byte LDS store per row block.
// Wave w computes output-channel tiles w, w + 4, ... for all 64 rows (16 tiles per pass).
#include "bq_common.h"

namespace bq {
namespace {

typedef __bf16 me_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 me_bf16x4 __attribute__((ext_vector_type(4)));
typedef float me_f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) me_f4u { float v[4]; };

constexpr int ME_TM = 64;           // rows per workgroup
constexpr int ME_THREADS = 256;     // four waves
constexpr int ME_KMAX = 512;        // input channels (rounded up to 32) a workgroup stages
constexpr int ME_NMAX = 256;        // widths of the BatchNorm layers
constexpr int ME_LDS_MAX = 160 * 1024;

struct MeArgs {
  bq_mlp_eval_desc d;
  int kin32;            // input channels rounded up to 32
  int off_b, off_st;    // LDS byte offsets of the second activation buffer and of the folded BatchNorm table
};

// one layer: out^T (n x 64) = W (n x k32) in^T; BN layers write bf16 rows to `out` (LDS), the tail writes fp32 to global
template <bool TAIL>
__device__ __forceinline__ void me_layer_run(const bq_mlp_eval_layer &L, const __bf16 *in, int sin, int k32, __bf16 *out,
                                             int sout, const float *s_tab, const float *t_tab, float *gout, long row0,
                                             long R, int wave, int lane) {
  const __bf16 *W = reinterpret_cast<const __bf16 *>(L.w);
  const int n = L.n, nct = (n + 15) >> 4;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  for (int ct0 = 0; ct0 < nct; ct0 += 16) {
    me_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[i][rb] = me_f32x4{0.f, 0.f, 0.f, 0.f};
    me_bf16x8 a[4], an[4];
    const me_bf16x8 zero8 = {};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nr = (ct0 + wave + 4 * i) * 16 + lr;
      a[i] = nr < n ? *reinterpret_cast<const me_bf16x8 *>(W + (long)nr * L.ldw + lk) : zero8;
      an[i] = zero8;
    }
    for (int k0 = 0; k0 < k32; k0 += 32) {
      if (k0 + 32 < k32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int nr = (ct0 + wave + 4 * i) * 16 + lr;
          an[i] = nr < n ? *reinterpret_cast<const me_bf16x8 *>(W + (long)nr * L.ldw + k0 + 32 + lk) : zero8;
        }
      }
      me_bf16x8 b[4];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) b[rb] = *reinterpret_cast<const me_bf16x8 *>(in + (rb * 16 + lr) * sin + k0 + lk);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (ct0 + wave + 4 * i < nct) {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb) acc[i][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[rb], acc[i][rb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = an[i];
    }
    // D[n = 4 (lane >> 4) + e][row = lane & 15] of every (channel tile, row block)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ct = ct0 + wave + 4 * i;
      if (ct >= nct) continue;
      const int nb = ct * 16 + (lane >> 4) * 4;
      if (!TAIL) {
        float sv[4], tv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] = s_tab[nb + e], tv[e] = t_tab[nb + e];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          me_bf16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float y = acc[i][rb][e] * sv[e] + tv[e];
            if (L.relu) y = y > 0.f ? y : 0.f;
            v[e] = (__bf16)y;
          }
          *reinterpret_cast<me_bf16x4 *>(out + (rb * 16 + lr) * sout + nb) = v;
        }
      } else {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          const long r = row0 + rb * 16 + lr;
          if (r >= R) continue;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (nb + e < n) {
              float y = acc[i][rb][e];
              if (L.bias) y = y + L.bias[nb + e];
              gout[r * n + nb + e] = y;
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(ME_THREADS) void mlp_eval_kernel(const MeArgs args) {
  extern __shared__ __attribute__((aligned(16))) unsigned char me_lds[];
  const bq_mlp_eval_desc &d = args.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)blockIdx.x * ME_TM;
  const long R = d.R;
  __bf16 *buf[2] = {reinterpret_cast<__bf16 *>(me_lds), reinterpret_cast<__bf16 *>(me_lds + args.off_b)};
  float *st = reinterpret_cast<float *>(me_lds + args.off_st);

  // ---- BatchNorm(eval) folded from the live parameters: s, t per channel of every layer
  for (int l = 0; l < d.n_layers; ++l) {
    const bq_mlp_eval_layer &L = d.layers[l];
    for (int c = tid; c < L.n; c += ME_THREADS) {
      const float g = L.gamma ? L.gamma[c] : 1.f, be = L.beta ? L.beta[c] : 0.f;
      const float s = g * (1.f / sqrtf(L.var[c] + L.eps));
      const float cb = L.bias ? L.bias[c] : 0.f;
      st[(2 * l) * ME_NMAX + c] = s;
      st[(2 * l + 1) * ME_NMAX + c] = be + (cb - L.mean[c]) * s;
    }
  }

  // ---- input rows -> LDS buffer 0 (row stride kin32 + 8), zero beyond the input channels and beyond R
  const int kin32 = args.kin32, s0 = kin32 + 8;
  __bf16 *x0 = buf[0];
  if (d.xyz) {
    // grouped form: row pos = (b * M + j) * S + k -> [(xyz[idx] - new_xyz[j]) (/ radius), feats[b, idx]]
    const int C = d.C, S = d.S, M = d.M, Np = d.N;
    const bool vec = (C & 3) == 0 && C <= 256;
    for (int h = 0; h < 2; ++h) {
      const int rbase = wave * 16 + h * 8;
      const long pmine = row0 + rbase + (lane & 7);
      const int myid = (lane < 8 && pmine < R) ? d.idx[pmine] : 0;
      if (vec) {
        me_f4u fv[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const long pos = row0 + rbase + r;
          const int id = __shfl(myid, r);
          if (pos < R && lane * 4 < C) {
            const int b = (int)(pos / S / M);
            fv[r] = *reinterpret_cast<const me_f4u *>(d.feats + (long)b * d.f_bs + (long)id * d.f_rs + lane * 4);
          }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const long pos = row0 + rbase + r;
          __bf16 *dst = x0 + (rbase + r) * s0;
          if (pos < R && lane * 4 < C) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[3 + lane * 4 + e] = (__bf16)fv[r].v[e];
          }
        }
      } else {
        for (int r = 0; r < 8; ++r) {
          const long pos = row0 + rbase + r;
          const int id = __shfl(myid, r);
          if (pos >= R) continue;
          const int b = (int)(pos / S / M);
          const float *f = d.feats + (long)b * d.f_bs + (long)id * d.f_rs;
          __bf16 *dst = x0 + (rbase + r) * s0;
          for (int c = lane; c < C; c += 64) dst[3 + c] = (__bf16)f[c];
        }
      }
      // coordinates (lanes 0..23: row lane / 3, axis lane % 3) and the zero padding
      const int idc = __shfl(myid, lane < 24 ? lane / 3 : 0);
      if (lane < 24) {
        const int r = lane / 3, ax = lane - r * 3;
        const long pos = row0 + rbase + r;
        if (pos < R) {
          const long bj = pos / S;
          const int b = (int)(bj / M);
          const int id = idc;
          float v = d.xyz[((long)b * Np + id) * 3 + ax] - d.new_xyz[bj * 3 + ax];
          if (d.normalize) v /= d.radius;
          x0[(rbase + r) * s0 + ax] = (__bf16)v;
        }
      }
      for (int r = 0; r < 8; ++r) {
        const long pos = row0 + rbase + r;
        __bf16 *dst = x0 + (rbase + r) * s0;
        for (int c = (pos < R ? 3 + C : 0) + lane; c < kin32; c += 64) dst[c] = (__bf16)0.f;
      }
    }
  } else {
    // rows form: 16-byte chunks of bf16 rows (K % 8 == 0, ldx % 8 == 0, 16-byte aligned base)
    const int K = d.K, cpr = kin32 / 8, kc = K / 8;
    const __bf16 *X = reinterpret_cast<const __bf16 *>(d.x);
    for (int q = tid; q < ME_TM * cpr; q += ME_THREADS) {
      const int r = q / cpr, c = q - r * cpr;
      uint4 v = {0u, 0u, 0u, 0u};
      if (c < kc && row0 + r < R) v = *reinterpret_cast<const uint4 *>(X + (row0 + r) * d.ldx + c * 8);
      *reinterpret_cast<uint4 *>(x0 + r * s0 + c * 8) = v;
    }
  }
  __syncthreads();

  // ---- the BatchNorm layers, LDS to LDS
  int sin = s0, k32 = kin32;
  for (int l = 0; l < d.n_layers; ++l) {
    const bq_mlp_eval_layer &L = d.layers[l];
    me_layer_run<false>(L, buf[l & 1], sin, k32, buf[(l + 1) & 1], L.n + 8, st + (2 * l) * ME_NMAX,
                        st + (2 * l + 1) * ME_NMAX, nullptr, row0, R, wave, lane);
    __syncthreads();
    sin = L.n + 8;
    k32 = L.n;
  }
  const int nl = d.n_layers;
  const __bf16 *last = buf[nl & 1];
  if (d.has_tail) {
    me_layer_run<true>(d.tail, last, sin, k32, nullptr, 0, nullptr, nullptr, reinterpret_cast<float *>(d.out), row0, R,
                       wave, lane);
    return;
  }
  const int n = k32, cpr = n / 8;
  __bf16 *O = reinterpret_cast<__bf16 *>(d.out);
  if (d.pool) {
    // max over each run of S rows (a tile holds 64 / S whole groups: R and row0 are multiples of S)
    const int S = d.S, groups = ME_TM / S;
    for (int q = tid; q < groups * cpr; q += ME_THREADS) {
      const int g = q / cpr, c = q - g * cpr;
      if (row0 + g * S >= R) continue;
      me_bf16x8 m = *reinterpret_cast<const me_bf16x8 *>(last + (g * S) * sin + c * 8);
      for (int r = 1; r < S; ++r) {
        const me_bf16x8 v = *reinterpret_cast<const me_bf16x8 *>(last + (g * S + r) * sin + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = (float)v[e] > (float)m[e] ? v[e] : m[e];
      }
      *reinterpret_cast<me_bf16x8 *>(O + (row0 / S + g) * n + c * 8) = m;
    }
  } else {
    for (int q = tid; q < ME_TM * cpr; q += ME_THREADS) {
      const int r = q / cpr, c = q - r * cpr;
      if (row0 + r < R)
        *reinterpret_cast<uint4 *>(O + (row0 + r) * n + c * 8) = *reinterpret_cast<const uint4 *>(last + r * sin + c * 8);
    }
  }
}

int me_check_layer(const bq_mlp_eval_layer &L, int k32, bool tail, int l) {
  BQ_REQUIRE(L.w && ((uintptr_t)L.w % 16) == 0, BQ_EINVAL, "mlp_eval: layer %d: null or misaligned weight", l);
  BQ_REQUIRE(L.ldw >= k32 && L.ldw % 8 == 0, BQ_EINVAL, "mlp_eval: layer %d: weight row stride %d for %d inputs", l, L.ldw,
             k32);
  if (tail) {
    BQ_REQUIRE(L.n >= 1 && L.n <= 4096, BQ_EINVAL, "mlp_eval: tail width %d", L.n);
  } else {
    BQ_REQUIRE(L.n >= 32 && L.n <= ME_NMAX && L.n % 32 == 0, BQ_EINVAL, "mlp_eval: layer %d: width %d (multiples of 32 up to %d)",
               l, L.n, ME_NMAX);
    BQ_REQUIRE(L.mean && L.var, BQ_EINVAL, "mlp_eval: layer %d: null running statistics", l);
  }
  return BQ_OK;
}

}  // namespace
}  // namespace bq

using namespace bq;

extern "C" int bq_mlp_eval(const bq_mlp_eval_desc *d, void *stream) {
  BQ_REQUIRE(d, BQ_EINVAL, "mlp_eval: null descriptor");
  BQ_REQUIRE(d->n_layers >= 1 && d->n_layers <= 3, BQ_EINVAL, "mlp_eval: %d layers (1..3)", d->n_layers);
  BQ_REQUIRE(d->R >= 0, BQ_EINVAL, "mlp_eval: bad extents");
  BQ_REQUIRE(d->out, BQ_EINVAL, "mlp_eval: null output");
  int kin;
  if (d->xyz) {
    BQ_REQUIRE(d->B >= 0 && d->C >= 0 && d->N >= 0 && d->M >= 0, BQ_EINVAL, "mlp_eval: bad extents");
    BQ_REQUIRE(d->S == 16 || d->S == 32 || d->S == 64, BQ_EINVAL, "mlp_eval: nsample %d (16, 32 or 64)", d->S);
    BQ_REQUIRE(d->R == (long)d->B * d->M * d->S, BQ_EINVAL, "mlp_eval: rows %ld != B M S", d->R);
    BQ_REQUIRE(d->new_xyz && d->idx && (d->feats || d->C == 0), BQ_EINVAL, "mlp_eval: null pointer");
    BQ_REQUIRE(d->C == 0 || (d->f_rs >= d->C && d->f_bs >= 0), BQ_EINVAL, "mlp_eval: feature strides");
    BQ_REQUIRE(!d->x, BQ_EINVAL, "mlp_eval: both input forms given");
    kin = 3 + d->C;
    if (d->C % 4 == 0 && d->C > 0 && d->C <= 256)
      BQ_REQUIRE(((uintptr_t)d->feats % 4) == 0, BQ_EINVAL, "mlp_eval: misaligned features");
  } else {
    BQ_REQUIRE(d->x, BQ_EINVAL, "mlp_eval: null pointer");
    BQ_REQUIRE(!d->pool, BQ_EINVAL, "mlp_eval: pooling needs the grouped form");
    BQ_REQUIRE(d->K >= 8 && d->K % 8 == 0 && d->ldx >= d->K && d->ldx % 8 == 0 && ((uintptr_t)d->x % 16) == 0, BQ_EINVAL,
               "mlp_eval: rows of %d channels, stride %ld (multiples of 8, 16-byte aligned)", d->K, d->ldx);
    kin = d->K;
  }
  const int kin32 = (kin + 31) / 32 * 32;
  BQ_REQUIRE(kin32 <= ME_KMAX, BQ_ELIMIT, "mlp_eval: %d input channels (at most %d)", kin, ME_KMAX);
  BQ_REQUIRE(!(d->pool && d->has_tail), BQ_EINVAL, "mlp_eval: pooling and a tail");
  int k32 = kin32;
  for (int l = 0; l < d->n_layers; ++l) {
    const int st = me_check_layer(d->layers[l], k32, false, l);
    if (st != BQ_OK) return st;
    k32 = d->layers[l].n;
  }
  if (d->has_tail) {
    const int st = me_check_layer(d->tail, k32, true, 3);
    if (st != BQ_OK) return st;
  } else {
    BQ_REQUIRE(((uintptr_t)d->out % 16) == 0, BQ_EINVAL, "mlp_eval: misaligned output");
  }
  // LDS: buffer 0 holds the input tile and the second layer's output, buffer 1 the first and third layers' outputs
  const int n0 = d->layers[0].n, n1 = d->n_layers > 1 ? d->layers[1].n : 0, n2 = d->n_layers > 2 ? d->layers[2].n : 0;
  const int sa = (kin32 + 8) > (n1 + 8) ? kin32 + 8 : n1 + 8, sb = (n0 > n2 ? n0 : n2) + 8;
  MeArgs a;
  a.d = *d;
  a.kin32 = kin32;
  a.off_b = ME_TM * sa * 2;
  a.off_st = a.off_b + ME_TM * sb * 2;
  const int lds = a.off_st + 6 * ME_NMAX * 4;
  BQ_REQUIRE(lds <= ME_LDS_MAX, BQ_ELIMIT, "mlp_eval: %d bytes of LDS", lds);
  if (d->R == 0) return BQ_OK;
  static bool lds_reserved = false;   // once: keeps the launch path free of driver calls
  if (!lds_reserved) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(mlp_eval_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, ME_LDS_MAX);
    if (e != hipSuccess) { set_error("mlp_eval: cannot reserve LDS: %s", hipGetErrorString(e)); return (int)e; }
    lds_reserved = true;
  }
  const long blocks = (d->R + ME_TM - 1) / ME_TM;
  BQ_REQUIRE(blocks < (1L << 31), BQ_ELIMIT, "mlp_eval: %ld rows", d->R);
  hipLaunchKernelGGL(mlp_eval_kernel, dim3((unsigned)blocks), dim3(ME_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("mlp_eval");
}
