// Detection mAP on the device -- the reference's utils/eval_det.py (eval_det_cls :57-141, voc_ap :4-35, the non-07 metric)
// over utils/box_util.py:112-123 box3d_iou, as lib/ap_helper.py:225-278 APCalculator drives them.  The reference walks every
// detection in Python with an inner Python loop over the ground-truth boxes; a detection's verdict depends only on the
// higher-scored detections of its own (class, scene), so here one wave matches one (class, scene) segment and the global
// confidence order is only needed for the cumulative sums, which one workgroup per (class, threshold) forms.
// All arithmetic in double, every product and sum rounded separately: the IoU equals numpy's bit for bit.
#include <math.h>

#include "bq_common.h"

namespace bq {

constexpr int AP_MAX_T = 4;            // thresholds per matching pass
constexpr int AP_MAX_SEG_GT = 2048;    // ground-truth boxes per segment: lane l owns l, l + 64, ... as bits of one u32 per threshold

struct ApThresholds {
  double v[AP_MAX_T];
};

struct ApBox {
  double x0, y0, z0, x1, y1, z1, vol;
};

__device__ __forceinline__ ApBox ap_load_box(const double *__restrict__ p) {
#pragma clang fp contract(off)
  ApBox b;
  b.x0 = p[0], b.y0 = p[1], b.z0 = p[2], b.x1 = p[3], b.y1 = p[4], b.z1 = p[5];
  b.vol = ((b.x1 - b.x0) * (b.y1 - b.y0)) * (b.z1 - b.z0);
  return b;
}

// box_util.py:114-123: inter = max(xB-xA, 0) * max(yB-yA, 0) * max(zB-zA, 0); iou = inter / (v1 + v2 - inter + 1e-8)
__device__ __forceinline__ double ap_iou(const ApBox &a, const ApBox &b) {
#pragma clang fp contract(off)
  const double xA = fmax(a.x0, b.x0), yA = fmax(a.y0, b.y0), zA = fmax(a.z0, b.z0);
  const double xB = fmin(a.x1, b.x1), yB = fmin(a.y1, b.y1), zB = fmin(a.z1, b.z1);
  const double dx = fmax(xB - xA, 0.0), dy = fmax(yB - yA, 0.0), dz = fmax(zB - zA, 0.0);
  const double inter = __dmul_rn(__dmul_rn(dx, dy), dz);
  const double den = __dadd_rn(__dsub_rn(__dadd_rn(a.vol, b.vol), inter), 1e-8);
  return inter / den;
}

// ---- greedy matching, one wave per (class, scene) segment (eval_det.py:102-129) -----------------------------------------
// The caller ordered the segment's detections by (score descending, list position ascending).  Lane l evaluates the
// ground-truth boxes l, l + 64, ...; a fixed butterfly gives the best overlap, equal overlaps resolving to the LOWEST
// index (the reference updates on strict >).  Only that box is considered: when it is taken the detection is a false
// positive, whatever else clears the threshold.  Taken flags: bit s of taken[t] in lane l = box s * 64 + l, threshold t.
// Results are parked in lane (position % 64) and leave with one coalesced store per 64 detections.
__global__ __launch_bounds__(256) void ap_match_kernel(const double *__restrict__ box_tab, const int *__restrict__ det_box,
                                                       const double *__restrict__ gt_tab, const int *__restrict__ seg_det,
                                                       const int *__restrict__ seg_gt, unsigned char *__restrict__ tp,
                                                       double *__restrict__ ovmax, int *__restrict__ jmax, ApThresholds thr,
                                                       int Nb, int D, int G, int S, int T) {
  const int lane = threadIdx.x & 63;
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= S) return;
  const int d0 = seg_det[seg], d1 = seg_det[seg + 1], g0 = seg_gt[seg], g1 = seg_gt[seg + 1];
  if (d0 < 0 || d1 > D || d1 < d0 || g0 < 0 || g1 > G || g1 < g0) return;       // malformed offsets: touch nothing
  const int ng = g1 - g0;
  const bool too_many = ng > AP_MAX_SEG_GT;      // beyond the caller's declared bound: marked, not matched
  const int nslot = too_many ? 0 : (ng + 63) >> 6;
  unsigned taken[AP_MAX_T] = {0u, 0u, 0u, 0u};
  // the common segment has at most 64 boxes: lane l keeps box l in registers
  ApBox mine = {0, 0, 0, 0, 0, 0, 0};
  if (lane < ng && nslot > 0) mine = ap_load_box(gt_tab + (long)(g0 + lane) * 6);
  double keep_ov = 0.0;
  int keep_j = 0;
  unsigned keep_tp = 0u;
  for (int d = d0; d < d1; ++d) {
    const int bi = det_box[d];
    double best = -INFINITY;
    int bj = 0x7fffffff;
    if (bi >= 0 && bi < Nb && nslot > 0) {
      const ApBox a = ap_load_box(box_tab + (long)bi * 6);
      if (lane < ng) {
        const double o = ap_iou(a, mine);
        if (o > best) best = o, bj = lane;
      }
      for (int s = 1; s < nslot; ++s) {
        const int j = s * 64 + lane;
        if (j < ng) {
          const double o = ap_iou(a, ap_load_box(gt_tab + (long)(g0 + j) * 6));
          if (o > best) best = o, bj = j;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(best, off);
      const int j = __shfl_xor(bj, off);
      if (o > best || (o == best && j < bj)) best = o, bj = j;
    }
    if (bj == 0x7fffffff) bj = -1;                 // no ground truth (or every overlap NaN): ovmax stays -inf
    if (too_many) best = NAN, bj = -2;
    unsigned bits = 0u;
#pragma unroll
    for (int t = 0; t < AP_MAX_T; ++t) {
      if (t < T && bj >= 0 && best > thr.v[t]) {
        const unsigned m = (unsigned)__shfl((int)taken[t], bj & 63);
        if (!((m >> (bj >> 6)) & 1u)) {
          bits |= 1u << t;
          if (lane == (bj & 63)) taken[t] |= 1u << (bj >> 6);
        }
      }
    }
    const int k = (d - d0) & 63;
    if (lane == k) keep_ov = best, keep_j = bj, keep_tp = bits;
    if (k == 63 || d == d1 - 1) {
      const int base = d - k;
      if (lane <= k) {
        ovmax[base + lane] = keep_ov;
        jmax[base + lane] = keep_j;
#pragma unroll
        for (int t = 0; t < AP_MAX_T; ++t)
          if (t < T) tp[(long)t * D + base + lane] = (unsigned char)((keep_tp >> t) & 1u);
      }
    }
  }
}

// ---- precision / recall curve and AP, one workgroup per (class, threshold) (eval_det.py:131-139, voc_ap :20-34) ------
// tp in curve order: (class, score descending, scene ascending, list position ascending).  Forward: inclusive scans in
// chunks of 256 (integers, exact in double), rec = tp / (npos + 1e-8), prec = tp / max(tp + fp, eps).  Backward: the
// precision envelope (reverse running maximum, sentinel 0 behind the last element) and the terms
// (mrec[i+1] - mrec[i]) * mpre[i+1] where recall changes; the sentinel pair (1 - rec[n-1]) * 0 contributes nothing.
// Thread t sums the terms of positions t, t + 256, ... from the last chunk to the first, then a fixed tree over the 256
// partial sums: the same bits on every run.
__global__ __launch_bounds__(256) void ap_curve_kernel(const unsigned char *__restrict__ tp, const int *__restrict__ cls_off,
                                                       const double *__restrict__ npos, double *__restrict__ rec,
                                                       double *__restrict__ prec, double *__restrict__ ap,
                                                       double *__restrict__ last_recall, int D, int C, int T) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[4];
  __shared__ double s_max[4];
  __shared__ double s_acc[256];
  const int c = blockIdx.x, tt = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c0 = cls_off[c], c1 = cls_off[c + 1];
  if (c0 < 0 || c1 > D || c1 < c0) {               // malformed offsets: touch nothing but the summary
    if (t == 0) ap[(long)c * T + tt] = NAN, last_recall[(long)c * T + tt] = NAN;
    return;
  }
  const int n = c1 - c0;
  const unsigned char *tpr = tp + (long)tt * D + c0;
  double *recr = rec + (long)tt * D + c0, *precr = prec + (long)tt * D + c0;
  const double den = npos[c] + 1e-8;
  const int nchunk = (n + 255) >> 8;
  int carry = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int i = ch * 256 + t;
    int x = i < n ? (int)tpr[i] : 0;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_cnt[w] = x;
    __syncthreads();
    int before = carry;
    for (int k = 0; k < 4; ++k) {
      if (k < w) before += s_cnt[k];
      carry += s_cnt[k];
    }
    if (i < n) {
      const double tpc = (double)(before + x), fpc = (double)(i + 1 - (before + x));
      const double r = tpc / den;
      recr[i] = r;
      precr[i] = tpc / fmax(tpc + fpc, 2.220446049250313e-16);
      if (i == n - 1) last_recall[(long)c * T + tt] = r;
    }
    __syncthreads();
  }
  // (the block's own rec / prec stores are visible to all its threads after the barrier above)
  double acc = 0.0, tail = 0.0;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int i = ch * 256 + t;
    double v = i < n ? precr[i] : 0.0;
    for (int off = 1; off < 64; off <<= 1) {
      const double y = __shfl_down(v, off);
      if (lane + off < 64) v = fmax(v, y);
    }
    if (lane == 0) s_max[w] = v;
    __syncthreads();
    double env = fmax(v, tail);
    for (int k = 0; k < 4; ++k) {
      if (k > w) env = fmax(env, s_max[k]);
      tail = fmax(tail, s_max[k]);
    }
    if (i < n) {
      const double r = recr[i], rp = i > 0 ? recr[i - 1] : 0.0;
      const double term = r != rp ? (r - rp) * env : 0.0;
      acc = acc + term;
    }
    __syncthreads();
  }
  s_acc[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) s_acc[t] = s_acc[t] + s_acc[t + s];
    __syncthreads();
  }
  if (t == 0) {
    ap[(long)c * T + tt] = s_acc[0];
    if (n == 0) last_recall[(long)c * T + tt] = 0.0;
  }
}

}  // namespace bq

using namespace bq;

extern "C" int bq_ap_match(
    const double *box_tab, const int *det_box, const double *gt_tab, const int *seg_det, const int *seg_gt,
    const double *thresholds, unsigned char *tp, double *ovmax, int *jmax, int Nb, int D, int G, int S, int T,
    int max_seg_gt, void *stream) {
  BQ_REQUIRE(T >= 1 && T <= AP_MAX_T, BQ_ELIMIT, "ap_match: T = %d outside 1..%d", T, AP_MAX_T);
  BQ_REQUIRE(max_seg_gt >= 0 && max_seg_gt <= AP_MAX_SEG_GT, BQ_ELIMIT,
             "ap_match: %d ground-truth boxes in one segment, limit %d", max_seg_gt, AP_MAX_SEG_GT);
  BQ_REQUIRE(Nb >= 0 && D >= 0 && G >= 0 && S >= 0, BQ_EINVAL, "ap_match: bad extents");
  BQ_REQUIRE(thresholds && seg_det && seg_gt, BQ_EINVAL, "ap_match: null pointer");
  BQ_REQUIRE(D == 0 || (box_tab && det_box && tp && ovmax && jmax && Nb > 0), BQ_EINVAL, "ap_match: null pointer");
  BQ_REQUIRE(G == 0 || gt_tab, BQ_EINVAL, "ap_match: null pointer");
  if (S == 0 || D == 0) return BQ_OK;
  ApThresholds thr = {{0, 0, 0, 0}};
  for (int t = 0; t < T; ++t) thr.v[t] = thresholds[t];
  hipLaunchKernelGGL(ap_match_kernel, dim3((S + 3) / 4), dim3(256), 0, (hipStream_t)stream, box_tab, det_box, gt_tab,
                     seg_det, seg_gt, tp, ovmax, jmax, thr, Nb, D, G, S, T);
  return check_launch("ap_match");
}

extern "C" int bq_ap_curve(
    const unsigned char *tp, const int *cls_off, const double *npos, double *rec, double *prec, double *ap,
    double *last_recall, int D, int C, int T, void *stream) {
  BQ_REQUIRE(T >= 1 && T <= AP_MAX_T, BQ_ELIMIT, "ap_curve: T = %d outside 1..%d", T, AP_MAX_T);
  BQ_REQUIRE(D >= 0 && C >= 0 && C <= 65535, BQ_EINVAL, "ap_curve: bad extents");
  BQ_REQUIRE(cls_off && npos && ap && last_recall, BQ_EINVAL, "ap_curve: null pointer");
  BQ_REQUIRE(D == 0 || (tp && rec && prec), BQ_EINVAL, "ap_curve: null pointer");
  if (C == 0) return BQ_OK;
  hipLaunchKernelGGL(ap_curve_kernel, dim3(C, T), dim3(256), 0, (hipStream_t)stream, tp, cls_off, npos, rec, prec, ap,
                     last_recall, D, C, T);
  return check_launch("ap_curve");
}
