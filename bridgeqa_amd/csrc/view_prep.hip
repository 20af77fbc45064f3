// Image views prepared on the device: Pillow's 8-bit bicubic resize of an RGB byte image to (OH, OW), then ToTensor / Normalize
// by table, written as fp32 or bf16 in NCHW or patch-major order (include/bqhip_view.h; reference lib/dataset.py:130-142,
// utils/blip_utils.py:96-111).  One launch per batch.
//
// The values are integers and table entries: a pass computes clamp((2^21 + sum in[xmin + x] * k[x]) >> 22, 0, 255) in int32 from
// coefficients the host built in double; the horizontal pass runs first and its result is bytes; the value written is
// norm[channel][byte].  No float arithmetic touches a pixel, so the result is the host definition bit for bit.
//
// view_prep_kernel  one workgroup per (view of the batch, tile of tile_rows output rows).
//   1  the vertical table's windows of the tile's rows give the input rows y0 .. y1 the tile needs
//   2  horizontal pass of those rows into LDS as bytes, planar per row: img[row][channel][ox] (consecutive lanes take
//      consecutive ox, so the LDS write of a wave is one run of bytes and the vertical pass reads one run per tap)
//   3  barrier; vertical pass out of LDS, table lookup (the 768 entries sit in LDS too), store
//   With VEC = 4 (OW a multiple of 4, an aligned output) a thread carries four neighbouring ox through both passes: one dword
//   LDS write / read per four bytes and one 16-byte (fp32) or 8-byte (bf16) store per four values.  In patch-major order a patch
//   row is a run of `patch` contiguous elements; four neighbouring ox stay inside one (patch is then a multiple of 4).
//   VEC = 1 is the same code one ox at a time, for odd widths.
// Every index that comes from memory (view, table, window start and length, row count) is clamped or checked against the
// extents before it is used: see the header.
#include "bq_common.h"

namespace bq {

#ifndef BQ_VIEW_THREADS
#define BQ_VIEW_THREADS 1024   // (measured against 256 and 512: profiles/view_prep.md)
#endif
constexpr int VP_THREADS = BQ_VIEW_THREADS;
constexpr int VP_NORM_BYTES = 4096;                             // the (3, 256) table in front of the LDS image, fp32 at the most
constexpr int VP_HALF = 1 << (BQ_VIEW_PRECISION_BITS - 1);

struct vp_table {
  const int32_t *bounds;   // (out, 2): xmin, n
  const int32_t *coef;     // (out, ks)
  int ks;
  bool ok;
};

__device__ __forceinline__ int vp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// table `t` of the store, for `out` outputs: checked against the extent of tab, so that bounds / coef rows are inside it
__device__ __forceinline__ vp_table vp_get(const int32_t *__restrict__ tab, const int32_t *__restrict__ desc, int NT, long n_tab,
                                           long long t, int out) {
  const int32_t *d = desc + (long)vp_clamp((int)min(max(t, 0LL), (long long)(NT - 1)), 0, NT - 1) * BQ_VIEW_DESC;
  const long boff = d[0], coff = d[1];
  vp_table r;
  r.ks = d[2];
  r.ok = boff >= 0 && coff >= 0 && r.ks >= 1 && boff + 2L * out <= n_tab && coff + (long)out * r.ks <= n_tab;
  r.bounds = tab + boff;
  r.coef = tab + coff;
  return r;
}

// window of output `o`: first input index in [0, in - 1], length in [0, min(ks, in - first)]
__device__ __forceinline__ void vp_window(const vp_table &t, int o, int in, int &first, int &n) {
  first = vp_clamp(t.bounds[2 * o], 0, in - 1);
  n = vp_clamp(t.bounds[2 * o + 1], 0, min(t.ks, in - first));
}

__device__ __forceinline__ unsigned vp_byte(int acc) { return (unsigned)vp_clamp(acc >> BQ_VIEW_PRECISION_BITS, 0, 255); }

__device__ __forceinline__ void vp_store4(float *p, float a, float b, float c, float d) { *(float4 *)p = make_float4(a, b, c, d); }
__device__ __forceinline__ void vp_store4(unsigned short *p, unsigned short a, unsigned short b, unsigned short c,
                                          unsigned short d) {
  *(uint2 *)p = make_uint2((unsigned)a | ((unsigned)b << 16), (unsigned)c | ((unsigned)d << 16));
}

template <typename T, int VEC, bool PATCH>
__global__ __launch_bounds__(VP_THREADS) void view_prep_kernel(
    const unsigned char *__restrict__ pixels, long n_pixels, const long long *__restrict__ views, int NV,
    const int32_t *__restrict__ tab, const int32_t *__restrict__ desc, int NT, long n_tab, const long long *__restrict__ index,
    const T *__restrict__ norm, T *__restrict__ out, int OH, int OW, int tile_rows, int lds_rows, int tiles, int patch) {
  extern __shared__ unsigned vp_lds[];
  T *snorm = (T *)vp_lds;                                                   // (3, 256)
  unsigned char *img = (unsigned char *)vp_lds + VP_NORM_BYTES;             // (lds_rows, 3, OW) bytes
  const int tid = threadIdx.x;
  const long b = blockIdx.x / tiles;
  const int r0 = (int)(blockIdx.x % tiles) * tile_rows;
  const int th = min(tile_rows, OH - r0);
  const long long v = min(max(index[b], 0LL), (long long)(NV - 1));
  const long long *vw = views + v * BQ_VIEW_COLS;
  const long long base = vw[0];
  const int H = (int)vw[1], W = (int)vw[2];
  const vp_table ht = vp_get(tab, desc, NT, n_tab, vw[3], OW), vt = vp_get(tab, desc, NT, n_tab, vw[4], OH);
  if (!ht.ok || !vt.ok || H < 1 || W < 1 || H > 65536 || W > 65536 || base < 0 || base + 3LL * H * W > n_pixels)
    return;                                                                 // (uniform over the workgroup)
  for (int i = tid; i < 768; i += VP_THREADS) snorm[i] = norm[i];
  // 1: the input rows of this tile
  int y0 = H, y1 = 0;
  for (int r = 0; r < th; ++r) {
    int first, n;
    vp_window(vt, r0 + r, H, first, n);
    y0 = min(y0, first);
    y1 = max(y1, first + n);
  }
  const int nrows = vp_clamp(y1 - y0, 0, lds_rows);
  const int row3 = 3 * OW, OWv = OW / VEC;
  // 2: horizontal pass, input rows y0 .. y0 + nrows - 1 -> img
  const unsigned char *src = pixels + base + (long)y0 * W * 3;
  for (int i = tid; i < nrows * 3 * OWv; i += VP_THREADS) {
    const int q = i % OWv, t = i / OWv, c = t % 3, yr = t / 3;
    const unsigned char *srow = src + (long)yr * W * 3 + c;
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int ox = q * VEC + j;
      int first, n;
      vp_window(ht, ox, W, first, n);
      const int32_t *k = ht.coef + (long)ox * ht.ks;
      const unsigned char *p = srow + first * 3;
      int acc = VP_HALF;
      for (int x = 0; x < n; ++x) acc += (int)p[3 * x] * k[x];
      packed |= vp_byte(acc) << (8 * j);
    }
    unsigned char *dst = img + yr * row3 + c * OW + q * VEC;
    if constexpr (VEC == 4)
      *(unsigned *)dst = packed;
    else
      *dst = (unsigned char)packed;
  }
  __syncthreads();
  // 3: vertical pass, lookup, store
  const int pp = patch * patch, gw = PATCH ? OW / patch : 0;
  for (int i = tid; i < th * 3 * OWv; i += VP_THREADS) {
    const int q = i % OWv, t = i / OWv, yr = t % th, c = t / th;
    const int oy = r0 + yr, ox = q * VEC;
    int first, n;
    vp_window(vt, oy, H, first, n);
    const int rel = first - y0;                                  // >= 0: y0 is the smallest first of the tile
    n = max(min(n, nrows - rel), 0);
    const int32_t *k = vt.coef + (long)oy * vt.ks;
    const unsigned char *col = img + rel * row3 + c * OW + ox;
    int acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = VP_HALF;
    for (int x = 0; x < n; ++x) {
      const int kx = k[x];
      if constexpr (VEC == 4) {
        const unsigned w = *(const unsigned *)(col + x * row3);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += (int)((w >> (8 * j)) & 255u) * kx;
      } else {
        acc[0] += (int)col[x * row3] * kx;
      }
    }
    long o;
    if constexpr (PATCH)
      o = (((b * (OH / patch) + oy / patch) * gw + ox / patch) * 3 + c) * pp + (oy % patch) * patch + ox % patch;
    else
      o = ((b * 3 + c) * OH + oy) * OW + ox;
    const T *nc = snorm + c * 256;
    if constexpr (VEC == 4)
      vp_store4(out + o, nc[vp_byte(acc[0])], nc[vp_byte(acc[1])], nc[vp_byte(acc[2])], nc[vp_byte(acc[3])]);
    else
      out[o] = nc[vp_byte(acc[0])];
  }
}

}  // namespace bq

extern "C" int bq_view_prep(const unsigned char *pixels, long n_pixels, const long long *views, int NV, const int32_t *tab,
                            const int32_t *desc, int NT, long n_tab, const long long *index, int B, const void *norm, void *out, int OH, int OW,
                            int tile_rows, int lds_rows, int out_bf16, int patch, void *stream) {
  using namespace bq;
  BQ_REQUIRE(NV >= 1 && NT >= 1 && n_tab >= 1 && n_pixels >= 3 && B >= 0, BQ_EINVAL,
             "view_prep: bad extents (NV = %d views in %ld bytes, NT = %d tables of %ld entries, B = %d)", NV, n_pixels, NT, n_tab,
             B);
  BQ_REQUIRE(OH >= 1 && OW >= 1 && OH <= 16384 && OW <= 16384, BQ_EINVAL, "view_prep: output %d x %d outside [1, 16384]", OH, OW);
  BQ_REQUIRE(patch >= 0 && (patch == 0 || (OH % patch == 0 && OW % patch == 0)), BQ_EINVAL,
             "view_prep: patch = %d does not divide the output %d x %d", patch, OH, OW);
  BQ_REQUIRE(tile_rows >= 1 && lds_rows >= 1, BQ_EINVAL, "view_prep: bad tile (tile_rows = %d, lds_rows = %d)", tile_rows,
             lds_rows);
  const long lds = VP_NORM_BYTES + (((long)lds_rows * 3 * OW + 3) & ~3L);
  BQ_REQUIRE(lds <= BQ_VIEW_LDS_BYTES, BQ_EINVAL, "view_prep: lds_rows = %d rows of %d bytes need %ld bytes of LDS (limit %d)", lds_rows,
             3 * OW, lds, BQ_VIEW_LDS_BYTES);
  const long tiles = (OH + tile_rows - 1) / tile_rows;
  BQ_REQUIRE(tiles * B <= 0x7FFFFFFFL, BQ_ELIMIT, "view_prep: %ld workgroups (the grid holds 2^31 - 1)", tiles * B);
  if (B == 0) return BQ_OK;
  BQ_REQUIRE(pixels && views && tab && desc && index && norm && out, BQ_EINVAL, "view_prep: null pointer");
  const size_t elem = out_bf16 ? 2 : 4;
  const int vec4 = OW % 4 == 0 && ((size_t)out % (4 * elem)) == 0 && (patch == 0 || patch % 4 == 0);
  const dim3 grid((unsigned)(tiles * B));
  const auto launch = [&](auto elem) {   // elem: a value of the output's element type (bf16 travels as its 16 bits)
    using T = decltype(elem);
    with_flags(vec4, patch, [&](auto V4, auto PATCH) {
      hipLaunchKernelGGL((view_prep_kernel<T, decltype(V4)::value ? 4 : 1, decltype(PATCH)::value>), grid, dim3(VP_THREADS),
                         (size_t)lds, (hipStream_t)stream, pixels, n_pixels, views, NV, tab, desc, NT, n_tab, index,
                         (const T *)norm, (T *)out, OH, OW, tile_rows, lds_rows, (int)tiles, patch);
    });
  };
  if (out_bf16) launch((unsigned short)0); else launch(0.0f);
  return check_launch("view_prep");
}
