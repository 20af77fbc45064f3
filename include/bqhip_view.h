/* bqhip_view.h -- image views prepared on the device (csrc/view_prep.hip): Pillow's 8-bit bicubic resize, ToTensor / Normalize by
 * table, fp32 or bf16, NCHW or patch-major.  Additive to ABI 6: bqhip_fusion.h includes this file, BQHIP_ABI_VERSION does not
 * move, no existing entry point changes.  Same conventions as bqhip.h (raw device pointers, extents, a hipStream_t passed as
 * void*, int status, bq_last_error()).
 *
 * Restates Image.resize((OW, OH), BICUBIC) on an RGB byte image followed by ToTensor and Normalize (reference lib/dataset.py:
 * 130-142, utils/blip_utils.py:96-111).  Every value is defined by integers and tables, so the output is bit exact:
 *
 *   out byte = clamp((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)     int32, horizontal pass first, bytes in between
 *   out value = norm[channel][out byte]
 *
 * The store: pixels (n_pixels bytes) = all views' (H, W, 3) bytes behind each other; views (NV, BQ_VIEW_COLS) long long =
 * first byte, H, W, index of the horizontal table, index of the vertical table.  tab (n_tab) int32 holds every table; desc (NT, BQ_VIEW_DESC)
 * int32 describes table t = offset of its bounds (out, 2) = (xmin, n) in tab, offset of its coefficients (out, ksize) in tab,
 * ksize, input extent.  A pass that does not change the extent is the table xmin = x, n = 1, k = 2^22: the byte itself.
 * The batch: index (B) long long in [0, NV); norm (3, 256) float (out_bf16 == 0) or bf16 bits (out_bf16 != 0).
 * out: (B, 3, OH, OW) with patch == 0, else (B, (OH / patch) (OW / patch), 3 patch patch) -- the element order of an unfold into
 * patch rows (channel, row in patch, column in patch); OH and OW must then be multiples of patch.
 * A workgroup takes tile_rows output rows of one view: the horizontal pass of the input rows they need goes into LDS as bytes
 * (lds_rows rows of 3 OW bytes, which the caller sizes from the vertical tables: 3 OW lds_rows + 4096 <= BQ_VIEW_LDS_BYTES),
 * the vertical pass reads them.  View indices, table indices, window bounds and row counts are clamped into their ranges by
 * the kernel, and a view or a table that does not lie inside n_pixels / n_tab is left unwritten: a bad value gives wrong
 * pixels, never an access outside the store, the tables or LDS.
 * Bad extents or a null pointer: BQ_EINVAL and a bq_last_error() text, nothing is launched. */
#ifndef BQHIP_VIEW_H
#define BQHIP_VIEW_H
#include "bqhip.h"

#define BQ_VIEW_COLS 5
#define BQ_VIEW_DESC 4
#define BQ_VIEW_LDS_BYTES 65536
#define BQ_VIEW_PRECISION_BITS 22

#ifdef __cplusplus
extern "C" {
#endif

BQ_API int bq_view_prep(const unsigned char *pixels, long n_pixels, const long long *views, int NV, const int32_t *tab,
                        const int32_t *desc, int NT, long n_tab, const long long *index, int B, const void *norm, void *out,
                        int OH, int OW, int tile_rows, int lds_rows, int out_bf16, int patch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_VIEW_H */
