// Training-scene preparation on the device: what ScannetQADataset.__getitem__ does per sample once the static features exist
// (reference lib/dataset.py:415-515, 537-573, 598-603, 803-816) -- draw N rows of a resident scene, flip / rotate x, y, z /
// translate points and boxes, build the vote labels -- as three launches per batch (include/bqhip_scene.h).
//
// The arithmetic is the reference's, operation for operation (the translation unit is built with -ffp-contract=off):
//   points  fp32 xyz; a flip negates; each rotation is xyz . R^T in fp64 as (x R[j][0] + y R[j][1]) + z R[j][2], rounded to fp32
//           after each of the three (the reference assigns np.dot's fp64 result into an fp32 array); then fp32(fp64(xyz) + t)
//   boxes   fp64 throughout, ALL G rows (the padding rows at -100 too), rounded to fp32 once at the end
//   votes   fp32: 0.5f * (min + max) over an instance's sampled, transformed xyz, minus the point
// The feature columns are copied bit for bit.
//
// scene_boxes_kernel   one thread per (sample, box row); thread 0 of a sample also fills the ref_* labels (the LAST box whose
//                      object id matches).  The same grid writes the initial value of every table entry.
// scene_sample_kernel  grid (workgroups per sample, sample); a workgroup takes tiles of 256 sampled points.  Per tile: thread p
//                      reads choice p and the row's xyz, transforms it, parks it in LDS and folds it into the workgroup's LDS
//                      table of per-instance min / max / first sample position (integer atomicMin / atomicMax on an
//                      order-preserving encoding of the float bits); then ALL lanes walk the tile's output, which is one
//                      contiguous run of 256 * D floats: element e belongs to point e / D, column e % D, so consecutive lanes
//                      store consecutive addresses and read consecutive columns of a source row (D = 135 is no multiple of 4:
//                      nothing here assumes an alignment).  After its tiles the workgroup flushes the entries it touched to
//                      the sample's global table with integer atomics.
// scene_vote_kernel    one thread per sampled point: its instance's entry, the first-position rule, 9 floats and the mask.
// Integer min / max do not depend on the order of arrival: two runs give the same bits.  There is no float atomic.
#include "bq_common.h"

namespace bq {

constexpr int SP_THREADS = 256;          // threads per workgroup = sampled points per tile
constexpr int SP_LDS_ENTRY = 7;          // min xyz, max xyz, first position (odd stride: neighbouring ids in different banks)
constexpr unsigned SP_NONE = 0xFFFFFFFFu;

// float -> unsigned whose order is the float order (-0 below +0; NaN is not expected in coordinates)
__device__ __forceinline__ unsigned sp_encode(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_decode(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }
// entry slot k: 0..2 take minima, 3..5 maxima, 6 the minimal position
__device__ __forceinline__ unsigned sp_initial(int k) { return (k >= 3 && k < 6) ? 0u : SP_NONE; }

__device__ __forceinline__ int sp_clamp(int v, int hi) { return min(max(v, 0), hi); }

// v . R^T for a row-major 3x3 R, every product and sum rounded on its own
__device__ __forceinline__ void sp_rotate(const double *__restrict__ R, double x, double y, double z, double &ox, double &oy,
                                          double &oz) {
  ox = (x * R[0] + y * R[1]) + z * R[2];
  oy = (x * R[3] + y * R[4]) + z * R[5];
  oz = (x * R[6] + y * R[7]) + z * R[8];
}

__device__ __forceinline__ void sp_point(const double *__restrict__ xf, float &x, float &y, float &z) {
  if (xf[0] < 0.0) x = -x;
  if (xf[1] < 0.0) y = -y;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double a, b, c;
    sp_rotate(xf + 2 + 9 * r, (double)x, (double)y, (double)z, a, b, c);
    x = (float)a;
    y = (float)b;
    z = (float)c;
  }
  x = (float)((double)x + xf[29]);
  y = (float)((double)y + xf[30]);
  z = (float)((double)z + xf[31]);
}

// rotate_aligned_boxes_along_axis: the centre turns; the extent along AXIS stays; each of the other two becomes twice the
// largest coordinate of the four turned corners (+-e1/2, +-e2/2, 0 on the axis).  AXIS = 2 is VoteNet's rotate_aligned_boxes.
// The ONE place that defines it on the device (the host states it in scene_data._rotate_boxes_along_axis).
template <int AXIS>
__device__ __forceinline__ void sp_rotate_box(const double *__restrict__ R, double (&c)[3], double (&e)[3]) {
  constexpr int P = AXIS == 0 ? 1 : 0, Q = AXIS == 2 ? 1 : 2;
  sp_rotate(R, c[0], c[1], c[2], c[0], c[1], c[2]);
  const double hp = e[P] / 2.0, hq = e[Q] / 2.0;
  double mp = 0.0, mq = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool pos_p = (i == 1 || i == 2), pos_q = (i >= 2);   // (-1,-1) (1,-1) (1,1) (-1,1)
    double v[3] = {0.0, 0.0, 0.0}, o[3];
    v[P] = pos_p ? hp : -hp;
    v[Q] = pos_q ? hq : -hq;
    sp_rotate(R, v[0], v[1], v[2], o[0], o[1], o[2]);
    mp = i == 0 ? o[P] : fmax(mp, o[P]);
    mq = i == 0 ? o[Q] : fmax(mq, o[Q]);
  }
  e[P] = 2.0 * mp;
  e[Q] = 2.0 * mq;
}

// row g of a sample's target_bboxes after augmentation, fp64
__device__ __forceinline__ void sp_box(const double *__restrict__ sb, int g, int nb, const double *__restrict__ xf, int augment,
                                       double (&c)[3], double (&e)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = g < nb ? sb[g * 8 + k] : -100.0;
    e[k] = g < nb ? sb[g * 8 + 3 + k] : -100.0;
  }
  if (!augment) return;
  if (xf[0] < 0.0) c[0] = -c[0];
  if (xf[1] < 0.0) c[1] = -c[1];
  sp_rotate_box<0>(xf + 2, c, e);
  sp_rotate_box<1>(xf + 11, c, e);
  sp_rotate_box<2>(xf + 20, c, e);
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = c[k] + xf[29 + k];
}

__global__ __launch_bounds__(SP_THREADS) void scene_boxes_kernel(
    const double *__restrict__ boxes, const int32_t *__restrict__ num_bbox, const int32_t *__restrict__ box_class,
    const double *__restrict__ mean_size, const int32_t *__restrict__ scene, const int32_t *__restrict__ object_id,
    const double *__restrict__ xf_all, float *__restrict__ target_bboxes, float *__restrict__ center_label,
    float *__restrict__ size_residual_label, float *__restrict__ heading_residual_label, float *__restrict__ box_label_mask,
    long long *__restrict__ heading_class_label, long long *__restrict__ size_class_label, long long *__restrict__ sem_cls_label,
    long long *__restrict__ ref_box_label, long long *__restrict__ num_bbox_out, long long *__restrict__ ref_obj_mask,
    float *__restrict__ ref_center_label, long long *__restrict__ ref_size_class_label,
    float *__restrict__ ref_size_residual_label, long long *__restrict__ flip_x, long long *__restrict__ flip_y,
    float *__restrict__ rot_mat, float *__restrict__ translation, unsigned *__restrict__ table, int S, int G, int NC, int B, long n_table,
    int augment) {
  const long i = (long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i < n_table) table[i] = sp_initial((int)(i % BQ_SCENE_ENTRY));
  if (i >= (long)B * G) return;
  const int b = (int)(i / G), g = (int)(i % G);
  const int s = sp_clamp(scene[b], S - 1);
  const double *sb = boxes + (long)s * G * 8;
  const int32_t *sc = box_class + (long)s * G;
  const int nb = sp_clamp(num_bbox[s], G);
  const double *xf = augment ? xf_all + (long)b * BQ_SCENE_XF : nullptr;
  const int oid = object_id[b];
  double c[3], e[3];
  sp_box(sb, g, nb, xf, augment, c, e);
  const int cls = g < nb ? sp_clamp(sc[g], NC - 1) : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    target_bboxes[i * 6 + k] = (float)c[k];
    target_bboxes[i * 6 + 3 + k] = (float)e[k];
    center_label[i * 3 + k] = (float)c[k];
    size_residual_label[i * 3 + k] = g < nb ? (float)(e[k] - mean_size[cls * 3 + k]) : 0.f;
  }
  heading_residual_label[i] = 0.f;
  box_label_mask[i] = g < nb ? 1.f : 0.f;
  heading_class_label[i] = 0;
  size_class_label[i] = cls;
  sem_cls_label[i] = cls;
  ref_box_label[i] = (g < nb && oid >= 0 && sb[g * 8 + 7] == (double)oid) ? 1 : 0;
  if (g != 0) return;
  // per-sample outputs
  num_bbox_out[b] = nb;
  ref_obj_mask[b] = oid >= 0 ? 1 : 0;
  int last = -1;
  if (oid >= 0)
    for (int j = 0; j < nb; ++j)
      if (sb[j * 8 + 7] == (double)oid) last = j;
  if (last >= 0) {
    sp_box(sb, last, nb, xf, augment, c, e);
    const int lc = sp_clamp(sc[last], NC - 1);
    ref_size_class_label[b] = lc;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ref_center_label[b * 3 + k] = (float)c[k];
      ref_size_residual_label[b * 3 + k] = (float)(e[k] - mean_size[lc * 3 + k]);
    }
  } else {
    ref_size_class_label[b] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ref_center_label[b * 3 + k] = ref_size_residual_label[b * 3 + k] = 0.f;
  }
  if (augment) {
    flip_x[b] = xf[0] < 0.0 ? -1 : 1;
    flip_y[b] = xf[1] < 0.0 ? -1 : 1;
#pragma unroll
    for (int k = 0; k < 9; ++k) rot_mat[b * 9 + k] = (float)xf[32 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) translation[b * 3 + k] = (float)xf[29 + k];
  }
}

__global__ __launch_bounds__(SP_THREADS) void scene_sample_kernel(
    const float *__restrict__ rows, const int32_t *__restrict__ inst, const long long *__restrict__ row_base,
    const int32_t *__restrict__ scene, const int32_t *__restrict__ choices, const double *__restrict__ xf_all,
    float *__restrict__ point_clouds, unsigned *__restrict__ table, int S, int N, int D, int T, int tiles_per_wg, int augment) {
  extern __shared__ unsigned sp_lds[];
  unsigned *tab = sp_lds;                                   // (T, SP_LDS_ENTRY)
  float *sx = (float *)(sp_lds + T * SP_LDS_ENTRY);         // (SP_THREADS, 3) transformed xyz of the tile
  int *srow = (int *)(sx + SP_THREADS * 3);                 // (SP_THREADS) source row of every point of the tile
  const int tid = threadIdx.x, b = blockIdx.y;
  const int s = sp_clamp(scene[b], S - 1);
  const long base = row_base[s];
  const int P = (int)(row_base[s + 1] - base);              // >= 1 (the store holds no empty scene)
  const double *xf = augment ? xf_all + (long)b * BQ_SCENE_XF : nullptr;
  const float *src = rows + base * D;
  for (int i = tid; i < T * SP_LDS_ENTRY; i += SP_THREADS) tab[i] = sp_initial(i % SP_LDS_ENTRY);
  __syncthreads();
  const int tiles = (N + SP_THREADS - 1) / SP_THREADS;
  const int t_end = min((int)(blockIdx.x + 1) * tiles_per_wg, tiles);
  for (int tile = blockIdx.x * tiles_per_wg; tile < t_end; ++tile) {
    const int j0 = tile * SP_THREADS;
    const int np = min(SP_THREADS, N - j0);
    if (tid < np) {
      const int j = j0 + tid;
      const int c = sp_clamp(choices[(long)b * N + j], P - 1);
      const float *r = src + (long)c * D;
      float x = r[0], y = r[1], z = r[2];
      if (augment) sp_point(xf, x, y, z);
      sx[tid * 3] = x;
      sx[tid * 3 + 1] = y;
      sx[tid * 3 + 2] = z;
      srow[tid] = c;
      unsigned *e = tab + sp_clamp(inst[base + c], T - 1) * SP_LDS_ENTRY;
      const unsigned ex = sp_encode(x), ey = sp_encode(y), ez = sp_encode(z);
      atomicMin(e, ex);
      atomicMin(e + 1, ey);
      atomicMin(e + 2, ez);
      atomicMax(e + 3, ex);
      atomicMax(e + 4, ey);
      atomicMax(e + 5, ez);
      atomicMin(e + 6, (unsigned)j);
    }
    __syncthreads();   // sx / srow of the tile written
    // (a wave per four rows with lane = column needs no division and measured slower: 0.43 against 0.30 ms per c2 batch,
    // profiles/scene_prep.md)
    float *dst = point_clouds + ((long)b * N + j0) * D;
    const int n = np * D;
#pragma unroll 4
    for (int i = tid; i < n; i += SP_THREADS) {
      const int p = (int)((unsigned)i / (unsigned)D), col = i - p * D;
      dst[i] = col < 3 ? sx[p * 3 + col] : src[(long)srow[p] * D + col];
    }
    __syncthreads();   // every read of sx / srow done before the next tile overwrites them
  }
  // the entries this workgroup touched (slot 6 took a position) -> the sample's table
  unsigned *gt = table + (long)b * T * BQ_SCENE_ENTRY;
  for (int id = tid; id < T; id += SP_THREADS) {
    const unsigned *e = tab + id * SP_LDS_ENTRY;
    if (e[6] == SP_NONE) continue;
    unsigned *g = gt + id * BQ_SCENE_ENTRY;
    atomicMin(g, e[0]);
    atomicMin(g + 1, e[1]);
    atomicMin(g + 2, e[2]);
    atomicMax(g + 3, e[3]);
    atomicMax(g + 4, e[4]);
    atomicMax(g + 5, e[5]);
    atomicMin(g + 6, e[6]);
  }
}

__global__ __launch_bounds__(SP_THREADS) void scene_vote_kernel(
    const int32_t *__restrict__ inst, const int32_t *__restrict__ sem, const unsigned char *__restrict__ votes_sem,
    const long long *__restrict__ row_base, const int32_t *__restrict__ scene, const int32_t *__restrict__ choices,
    const float *__restrict__ point_clouds, const unsigned *__restrict__ table, float *__restrict__ vote_label,
    long long *__restrict__ vote_label_mask, int S, int N, int D, int T, int L) {
  const int b = blockIdx.y, j = blockIdx.x * SP_THREADS + threadIdx.x;
  if (j >= N) return;
  const int s = sp_clamp(scene[b], S - 1);
  const long base = row_base[s];
  const int P = (int)(row_base[s + 1] - base);
  const int32_t *ch = choices + (long)b * N;
  const int c = sp_clamp(ch[j], P - 1);
  const unsigned *e = table + ((long)b * T + sp_clamp(inst[base + c], T - 1)) * BQ_SCENE_ENTRY;
  // the instance's first sampled point decides (its own entry was touched by this very point: e[6] <= j)
  const int first = (int)min(e[6], (unsigned)j);
  const int label = sem[base + sp_clamp(ch[first], P - 1)];
  const bool votes = label >= 0 && label < L && votes_sem[label] != 0;
  float v[3] = {0.f, 0.f, 0.f};
  if (votes) {
    const float *xyz = point_clouds + ((long)b * N + j) * D;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float center = 0.5f * (sp_decode(e[k]) + sp_decode(e[3 + k]));
      v[k] = center - xyz[k];
    }
  }
  float *out = vote_label + ((long)b * N + j) * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = v[k % 3];
  vote_label_mask[(long)b * N + j] = votes ? 1 : 0;
}

static int scene_common(const char *what, int S, int B, int T) {
  BQ_REQUIRE(S >= 1 && B >= 0, BQ_EINVAL, "%s: bad extents (S = %d scenes, B = %d samples)", what, S, B);
  BQ_REQUIRE(B <= 65535, BQ_ELIMIT, "%s: B = %d samples (the grid holds 65535)", what, B);
  BQ_REQUIRE(T >= 1 && T <= BQ_SCENE_MAX_IDS, BQ_EINVAL, "%s: T = %d table entries per sample outside [1, %d]", what, T,
             BQ_SCENE_MAX_IDS);
  return BQ_OK;
}

}  // namespace bq

extern "C" int bq_scene_boxes(const double *boxes, const int32_t *num_bbox, const int32_t *box_class, const double *mean_size,
                              const int32_t *scene, const int32_t *object_id, const double *xf, float *target_bboxes,
                              float *center_label, float *size_residual_label, float *heading_residual_label,
                              float *box_label_mask, long long *heading_class_label, long long *size_class_label,
                              long long *sem_cls_label, long long *ref_box_label, long long *num_bbox_out,
                              long long *ref_obj_mask, float *ref_center_label, long long *ref_size_class_label,
                              float *ref_size_residual_label, long long *flip_x, long long *flip_y, float *rot_mat,
                              float *translation, unsigned *table, int S, int G, int NC, int B, int T, int augment,
                              void *stream) {
  using namespace bq;
  const int st = scene_common("scene_boxes", S, B, T);
  if (st != BQ_OK) return st;
  BQ_REQUIRE(G >= 1 && G <= 65536 && NC >= 1, BQ_EINVAL, "scene_boxes: bad extents (G = %d box rows, NC = %d classes)", G, NC);
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(boxes && num_bbox && box_class && mean_size && scene && object_id && target_bboxes && center_label &&
                 size_residual_label && heading_residual_label && box_label_mask && heading_class_label && size_class_label &&
                 sem_cls_label && ref_box_label && num_bbox_out && ref_obj_mask && ref_center_label && ref_size_class_label &&
                 ref_size_residual_label && table,
             BQ_EINVAL, "scene_boxes: null pointer");
  BQ_REQUIRE(!augment || (xf && flip_x && flip_y && rot_mat && translation), BQ_EINVAL,
             "scene_boxes: augment needs xf, flip_x, flip_y, rot_mat and translation");
  const long n_table = (long)B * T * BQ_SCENE_ENTRY;
  const long n = n_table > (long)B * G ? n_table : (long)B * G;
  hipLaunchKernelGGL(scene_boxes_kernel, dim3((unsigned)((n + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0,
                     (hipStream_t)stream, boxes, num_bbox, box_class, mean_size, scene, object_id, xf, target_bboxes, center_label,
                     size_residual_label, heading_residual_label, box_label_mask, heading_class_label, size_class_label,
                     sem_cls_label, ref_box_label, num_bbox_out, ref_obj_mask, ref_center_label, ref_size_class_label,
                     ref_size_residual_label, flip_x, flip_y, rot_mat, translation, table, S, G, NC, B, n_table, augment ? 1 : 0);
  return check_launch("scene_boxes");
}

extern "C" int bq_scene_sample(const float *rows, const int32_t *inst, const long long *row_base, const int32_t *scene,
                               const int32_t *choices, const double *xf, float *point_clouds, unsigned *table, int S, int B,
                               int N, int D, int T, int augment, void *stream) {
  using namespace bq;
  const int st = scene_common("scene_sample", S, B, T);
  if (st != BQ_OK) return st;
  BQ_REQUIRE(N >= 0 && D >= 3 && D <= 65536, BQ_EINVAL, "scene_sample: bad extents (N = %d points, D = %d columns)", N, D);
  BQ_REQUIRE(N <= (1 << 24), BQ_ELIMIT, "scene_sample: N = %d sampled points (limit %d)", N, 1 << 24);
  if (B == 0 || N == 0) return BQ_OK;
  BQ_REQUIRE(rows && inst && row_base && scene && choices && point_clouds && table, BQ_EINVAL, "scene_sample: null pointer");
  BQ_REQUIRE(!augment || xf, BQ_EINVAL, "scene_sample: augment needs xf");
  // tiles per workgroup: about eight workgroups per compute unit before a workgroup takes a second tile (the LDS table is
  // initialised and flushed once per workgroup), eight tiles at the most
  const int tiles = (N + SP_THREADS - 1) / SP_THREADS;
  const long want = 8L * device_cus();
  long per = ((long)tiles * B + want - 1) / want;
  per = per < 1 ? 1 : (per > 8 ? 8 : per);
  const int wgs = (int)((tiles + per - 1) / per);
  const size_t lds = ((size_t)T * SP_LDS_ENTRY + SP_THREADS * 4) * sizeof(unsigned);   // <= 61440 bytes at T = 2048
  hipLaunchKernelGGL(scene_sample_kernel, dim3(wgs, B), dim3(SP_THREADS), lds, (hipStream_t)stream, rows, inst, row_base, scene,
                     choices, xf, point_clouds, table, S, N, D, T, (int)per, augment ? 1 : 0);
  return check_launch("scene_sample");
}

extern "C" int bq_scene_votes(const int32_t *inst, const int32_t *sem, const unsigned char *votes_sem, const long long *row_base,
                              const int32_t *scene, const int32_t *choices, const float *point_clouds, const unsigned *table,
                              float *vote_label, long long *vote_label_mask, int S, int B, int N, int D, int T, int L,
                              void *stream) {
  using namespace bq;
  const int st = scene_common("scene_votes", S, B, T);
  if (st != BQ_OK) return st;
  BQ_REQUIRE(N >= 0 && D >= 3 && D <= 65536 && L >= 1, BQ_EINVAL, "scene_votes: bad extents (N = %d, D = %d, L = %d)", N, D, L);
  BQ_REQUIRE(N <= (1 << 24), BQ_ELIMIT, "scene_votes: N = %d sampled points (limit %d)", N, 1 << 24);
  if (B == 0 || N == 0) return BQ_OK;
  BQ_REQUIRE(inst && sem && votes_sem && row_base && scene && choices && point_clouds && table && vote_label && vote_label_mask,
             BQ_EINVAL, "scene_votes: null pointer");
  hipLaunchKernelGGL(scene_vote_kernel, dim3((N + SP_THREADS - 1) / SP_THREADS, B), dim3(SP_THREADS), 0, (hipStream_t)stream,
                     inst, sem, votes_sem, row_base, scene, choices, point_clouds, table, vote_label, vote_label_mask, S, N, D, T,
                     L);
  return check_launch("scene_votes");
}
