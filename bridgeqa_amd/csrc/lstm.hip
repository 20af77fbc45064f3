// The LSTM recurrence of the question branch (reference models/lang_module.py:48-55, 95-99: nn.LSTM over a packed sequence),
// forward and backward, fp32 throughout.
//
// What is a matrix product over ALL time steps stays outside: Gx = x W_ih^T + b_ih + b_hh (forward), dX / dW_ih / dW_hh / the
// bias gradients (backward) are GEMMs and a column sum over dGx.  The kernels hold the part that is sequential in t.
//
// One workgroup of 4H threads owns one sequence from its first step to its last; nothing is communicated between workgroups
// (no grid barrier, no cooperative launch, no spin, no atomics).  The step count is len[b] clamped to [0, T_out]: a value
// every thread of the workgroup reads from the same address, so every __syncthreads() of the loop is reached by all waves.
// H in {128, 256} (a template parameter): 512 / 1024 threads.
//
// forward, step t (t = 0 .. n-1, or n-1 .. 0 with `reverse`), thread j = gate column (gate j / H in torch's order i f g o --
// wave-uniform, H is a multiple of 64):
//   pre[j] = Gx[b, t, j] + sum_k h[k] WT[k, j]      WT (H, 4H) = W_hh^T: lane j reads column j, coalesced over lanes; h from LDS
//   act[j] = sigmoid / tanh(pre[j]) -> LDS (and the saved gates);  threads j < H: c = f c + i g, h = o tanh(c) -> LDS, Y, cells
// The sum over k runs in four interleaved chains (k mod 4), added as (a0 + a1) + (a2 + a3); products and sums are rounded
// separately (-ffp-contract=off), expf / tanhf are the full-precision routines: tests/lstm_ref.py emulates exactly this order.
// Rows t >= n of Y are written as zeros here (the pad_packed_sequence contract); h_last is the state after the last step taken.
//
// backward walks the steps in the opposite order, threads k < H carry dh / dc:
//   dh = dY[b, t, k] + dh_rec[k] (+ dh_last[k] at the forward's last step);  tc = tanh(c_t)
//   do = dh tc;  dc += dh o (1 - tc^2);  di = dc g;  dg = dc i;  df = dc c_{t-1};  dc <- dc f
//   dGx[b, t] = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o)) -> LDS and global
//   dh_rec[k] = sum_r W_hh[r, k] dgate[r]: thread (q, k) sums the H rows of gate q (lane k reads W_hh (4H, H) coalesced), four
//   chains as above; thread k adds the four gates' partials as (p0 + p1) + (p2 + p3).
// Rows t >= n of dGx are written as zeros.
#include <math.h>

#include "bq_common.h"

namespace bq {

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_fwd_kernel(const float *__restrict__ Gx, const float *__restrict__ WT,
                                                         const int32_t *__restrict__ lens, float *__restrict__ Y,
                                                         float *__restrict__ h_last, float *__restrict__ gates,
                                                         float *__restrict__ cells, int T, int T_out, int reverse) {
  __shared__ float hs[H];
  __shared__ float act[4 * H];
  const int b = blockIdx.x, j = threadIdx.x;
  const int n = min(max(lens[b], 0), T_out);  // workgroup-uniform (T_out <= T: checked on the host)
  const float *gx = Gx + (long)b * T * 4 * H;
  float *y = Y + (long)b * T_out * H;
  const float *w = WT + j;
  const int gate = j / H;
  float c = 0.f, h = 0.f;
  if (j < H) hs[j] = 0.f;
  // the padding rows: no step reads them
  for (int i = n * H + j; i < T_out * H; i += 4 * H) y[i] = 0.f;
  __syncthreads();
  for (int s = 0; s < n; ++s) {
    const int t = reverse ? n - 1 - s : s;
    const float g_in = gx[(long)t * 4 * H + j];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
    for (int k = 0; k < H; k += 4) {
      a0 = a0 + hs[k] * w[(long)k * 4 * H];
      a1 = a1 + hs[k + 1] * w[(long)(k + 1) * 4 * H];
      a2 = a2 + hs[k + 2] * w[(long)(k + 2) * 4 * H];
      a3 = a3 + hs[k + 3] * w[(long)(k + 3) * 4 * H];
    }
    const float pre = g_in + ((a0 + a1) + (a2 + a3));
    const float a = gate == 2 ? tanhf(pre) : lstm_sigmoid(pre);
    act[j] = a;
    if (gates) gates[((long)b * T_out + t) * 4 * H + j] = a;
    __syncthreads();  // every act[] written; every read of hs[] of this step done
    if (j < H) {
      c = act[H + j] * c + act[j] * act[2 * H + j];
      h = act[3 * H + j] * tanhf(c);
      hs[j] = h;
      y[(long)t * H + j] = h;
      if (cells) cells[((long)b * T_out + t) * H + j] = c;
    }
    __syncthreads();  // hs[] of the next step written; act[] free again
  }
  if (j < H) h_last[(long)b * H + j] = h;
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_bwd_kernel(const float *__restrict__ dY, const float *__restrict__ dh_last,
                                                         const float *__restrict__ gates, const float *__restrict__ cells,
                                                         const float *__restrict__ W, const int32_t *__restrict__ lens,
                                                         float *__restrict__ dGx, int T_out, int reverse) {
  __shared__ float dg_s[4 * H];
  __shared__ float part[4 * H];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), T_out);  // workgroup-uniform
  const int q = tid / H, k = tid % H;
  float *dgx = dGx + (long)b * T_out * 4 * H;
  const float *gt = gates + (long)b * T_out * 4 * H;
  const float *ct = cells + (long)b * T_out * H;
  for (int i = n * 4 * H + tid; i < T_out * 4 * H; i += 4 * H) dgx[i] = 0.f;
  float dh_rec = 0.f, dc = 0.f;
  const float *w = W + (long)q * H * H + k;
  for (int s = 0; s < n; ++s) {
    // forward order was t = s' (or n-1-s' reversed), s' = 0..n-1; this walks s' = n-1..0
    const int sf = n - 1 - s;
    const int t = reverse ? n - 1 - sf : sf;
    if (tid < H) {
      float dh = dY ? dY[((long)b * T_out + t) * H + k] + dh_rec : dh_rec;
      if (s == 0 && dh_last) dh = dh + dh_last[(long)b * H + k];
      const float gi = gt[(long)t * 4 * H + k], gf = gt[(long)t * 4 * H + H + k], gg = gt[(long)t * 4 * H + 2 * H + k],
                  go = gt[(long)t * 4 * H + 3 * H + k];
      const float cc = ct[(long)t * H + k];
      float cp = 0.f;
      if (sf > 0) cp = ct[(long)(reverse ? t + 1 : t - 1) * H + k];
      const float tc = tanhf(cc);
      const float d_o = dh * tc;
      dc = dc + (dh * go) * (1.0f - tc * tc);
      const float di = dc * gg, dg = dc * gi, df = dc * cp;
      dc = dc * gf;
      const float ai = (di * gi) * (1.0f - gi), af = (df * gf) * (1.0f - gf), ag = dg * (1.0f - gg * gg),
                  ao = (d_o * go) * (1.0f - go);
      dg_s[k] = ai;
      dg_s[H + k] = af;
      dg_s[2 * H + k] = ag;
      dg_s[3 * H + k] = ao;
    }
    __syncthreads();  // dg_s[] of this step written
    dgx[(long)t * 4 * H + tid] = dg_s[tid];
    if (sf > 0) {  // (workgroup-uniform: the first forward step has no predecessor to send a gradient to)
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      const float *d = dg_s + q * H;
#pragma unroll 8
      for (int m = 0; m < H; m += 4) {
        a0 = a0 + d[m] * w[(long)m * H];
        a1 = a1 + d[m + 1] * w[(long)(m + 1) * H];
        a2 = a2 + d[m + 2] * w[(long)(m + 2) * H];
        a3 = a3 + d[m + 3] * w[(long)(m + 3) * H];
      }
      part[tid] = (a0 + a1) + (a2 + a3);
      __syncthreads();  // part[] written; every read of dg_s[] done
      if (tid < H) dh_rec = (part[k] + part[H + k]) + (part[2 * H + k] + part[3 * H + k]);
    }
    // (no third barrier: the next step writes dg_s[] after the barrier above, which every read of dg_s[] precedes, and
    // part[] after its own first barrier, which the reads of part[] precede; sf == 0 is the last step)
  }
}

static int lstm_common(const char *what, int B, int T_out, int H) {
  BQ_REQUIRE(B >= 0 && T_out >= 0, BQ_EINVAL, "%s: bad extents", what);
  BQ_REQUIRE(H == 128 || H == 256, BQ_EINVAL, "%s: hidden size %d (128 and 256 are built)", what, H);
  BQ_REQUIRE((long)B * T_out * 4 * H < (1L << 40), BQ_ELIMIT, "%s: too large", what);
  return BQ_OK;
}

}  // namespace bq

extern "C" int bq_lstm_fwd(const float *Gx, const float *WT, const int32_t *lens, float *Y, float *h_last, float *gates,
                           float *cells, int B, int T, int T_out, int H, int reverse, void *stream) {
  using namespace bq;
  const int st = lstm_common("lstm_fwd", B, T_out, H);
  if (st != BQ_OK) return st;
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(Gx && WT && lens && h_last && (Y || T_out == 0), BQ_EINVAL, "lstm_fwd: null pointer");
  BQ_REQUIRE(T_out <= T, BQ_EINVAL, "lstm_fwd: T_out %d > T %d", T_out, T);
  BQ_REQUIRE((gates == nullptr) == (cells == nullptr), BQ_EINVAL, "lstm_fwd: gates and cells are saved together");
  if (H == 128)
    hipLaunchKernelGGL(lstm_fwd_kernel<128>, dim3(B), dim3(512), 0, (hipStream_t)stream, Gx, WT, lens, Y, h_last, gates, cells,
                       T, T_out, reverse ? 1 : 0);
  else
    hipLaunchKernelGGL(lstm_fwd_kernel<256>, dim3(B), dim3(1024), 0, (hipStream_t)stream, Gx, WT, lens, Y, h_last, gates, cells,
                       T, T_out, reverse ? 1 : 0);
  return check_launch("lstm_fwd");
}

extern "C" int bq_lstm_bwd(const float *dY, const float *dh_last, const float *gates, const float *cells, const float *W,
                           const int32_t *lens, float *dGx, int B, int T_out, int H, int reverse, void *stream) {
  using namespace bq;
  const int st = lstm_common("lstm_bwd", B, T_out, H);
  if (st != BQ_OK) return st;
  if (B == 0 || T_out == 0) return BQ_OK;
  BQ_REQUIRE(gates && cells && W && lens && dGx, BQ_EINVAL, "lstm_bwd: null pointer");
  if (H == 128)
    hipLaunchKernelGGL(lstm_bwd_kernel<128>, dim3(B), dim3(512), 0, (hipStream_t)stream, dY, dh_last, gates, cells, W, lens, dGx,
                       T_out, reverse ? 1 : 0);
  else
    hipLaunchKernelGGL(lstm_bwd_kernel<256>, dim3(B), dim3(1024), 0, (hipStream_t)stream, dY, dh_last, gates, cells, W, lens, dGx,
                       T_out, reverse ? 1 : 0);
  return check_launch("lstm_bwd");
}
