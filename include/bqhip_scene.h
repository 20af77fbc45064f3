/* bqhip_scene.h -- training-scene preparation on the device (csrc/scene_prep.hip): sample, augment, vote labels.  Additive to
 * ABI 6: bqhip_fusion.h includes this file, BQHIP_ABI_VERSION does not move, no existing entry point changes.  Same conventions
 * as bqhip.h (raw device pointers, extents, a hipStream_t passed as void*, int status, bq_last_error()).
 *
 * Restates what ScannetQADataset.__getitem__ does per sample after the static features are built (reference lib/dataset.py:
 * 415-515, 537-573, 598-603, 803-816).  The three entry points are one batch's three launches, in this order on one stream:
 *
 *   bq_scene_boxes   one thread per (sample, box row), fp64, rounded to fp32 once; also writes the initial value of every entry
 *                    of `table` (so no memset precedes bq_scene_sample)
 *   bq_scene_sample  gathers the sampled rows, transforms xyz, folds xyz into `table` with integer atomicMin / atomicMax
 *   bq_scene_votes   reads `table` and the transformed xyz, writes vote_label / vote_label_mask
 *
 * The store (S scenes, ragged): rows (sum P, D) fp32, xyz first; inst / sem (sum P) int32; row_base (S + 1) = the first point of
 * every scene and the total; boxes (S, G, 8) fp64 = cx cy cz dx dy dz nyu40id object-id, the first num_bbox[s] <= G rows used;
 * box_class (S, G) int32 in [0, NC); mean_size (NC, 3) fp64; votes_sem (L) bytes: non-zero where a semantic id votes.
 * The batch: scene (B) int32 in [0, S); choices (B, N) int32 in [0, P_scene); object_id (B) int32, < 0 for none;
 * xf (B, BQ_SCENE_XF) fp64 = flip_x, flip_y (+-1), Rx, Ry, Rz (row-major 3x3 each), t (3), Rz Ry Rx (9).  augment == 0: a pure
 * gather -- xf is not read (may be NULL) and flip_x / flip_y / rot_mat / translation are not written (may be NULL).
 * table (B, T, BQ_SCENE_ENTRY) unsigned: per (sample, instance id) min xyz, max xyz in an order-preserving encoding and the
 * first sample position; T > the largest instance id of the store, T <= BQ_SCENE_MAX_IDS.
 * Scene indices, choices and instance ids are clamped into their ranges by the kernels: a bad value reads a wrong row, never
 * memory outside the store.  Bad extents or a null pointer: BQ_EINVAL and a bq_last_error() text, nothing is launched. */
#ifndef BQHIP_SCENE_H
#define BQHIP_SCENE_H
#include "bqhip.h"

#define BQ_SCENE_XF 41
#define BQ_SCENE_ENTRY 8
#define BQ_SCENE_MAX_IDS 2048

#ifdef __cplusplus
extern "C" {
#endif

BQ_API int bq_scene_boxes(const double *boxes, const int32_t *num_bbox, const int32_t *box_class, const double *mean_size,
                          const int32_t *scene, const int32_t *object_id, const double *xf, float *target_bboxes,
                          float *center_label, float *size_residual_label, float *heading_residual_label,
                          float *box_label_mask, long long *heading_class_label, long long *size_class_label,
                          long long *sem_cls_label, long long *ref_box_label, long long *num_bbox_out,
                          long long *ref_obj_mask, float *ref_center_label, long long *ref_size_class_label,
                          float *ref_size_residual_label, long long *flip_x, long long *flip_y, float *rot_mat,
                          float *translation, unsigned *table, int S, int G, int NC, int B, int T, int augment, void *stream);
BQ_API int bq_scene_sample(const float *rows, const int32_t *inst, const long long *row_base, const int32_t *scene,
                           const int32_t *choices, const double *xf, float *point_clouds, unsigned *table, int S, int B, int N,
                           int D, int T, int augment, void *stream);
BQ_API int bq_scene_votes(const int32_t *inst, const int32_t *sem, const unsigned char *votes_sem, const long long *row_base,
                          const int32_t *scene, const int32_t *choices, const float *point_clouds, const unsigned *table,
                          float *vote_label, long long *vote_label_mask, int S, int B, int N, int D, int T, int L,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_SCENE_H */
