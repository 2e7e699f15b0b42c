/*
 * smesh_eval.h -- scoring the fused mesh against ground truth, on the device: an extension of the C ABI in smesh.h.
 *
 * The reference's evaluation scores the fused mesh twice (eval-scannet/eval_scannet.py): per VERTEX (:108-112, :286-287) and per
 * PIXEL in a second render pass (:301-316) that gathers a (H,W,C) float image of annotations for every frame and feeds it to a
 * confusion-matrix metric.  The class-vector image is not needed: one int32 label per primitive (smesh_aggregator_labels), the
 * rendered index plane and the ground-truth label image give the same counts at about 5 bytes per pixel.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * Definitions (this project's; DESIGN.md "Confusion matrices").  A confusion matrix for C classes is uint64 [C, C + 1], row-major:
 *   M[g, p], p < C   samples with ground truth g and prediction p, both in [0, C)
 *   M[g, C]          samples with ground truth g and a DON'T-CARE prediction: a predicted label outside [0, C) (-1 included), a
 *                    pixel that no primitive covers, or a primitive index >= P.  They stay in the matrix as errors.
 *   ignored          samples whose ground truth lies outside [0, C) (negative values, 255 ...): they enter no cell.
 * All counts are integers: a result does not depend on launch shape, on the order of atomics or on how samples were batched.
 *
 * The label of a row of smesh_aggregator_get (float32): t = the sum of the row in ascending class order, starting from 0; the
 * label is the lowest c with the largest value, and -1 when t < dont_care_threshold -- the rule of smesh_vertices.h for a vertex.
 *
 * Conventions are those of smesh_labels.h: images are (W,H) with y fastest, strides in ELEMENTS and >= 0 (NULL: dense), ground
 * truth is of any SMESH_LBL_* dtype, every function returns a status, SMESH_ERR_INVALID (with a message, and with the matrix
 * unchanged) for a bad dtype, stride, shape, P or device.  HOST arrays are consumed before a call returns; DEVICE arrays -- and
 * `prim_labels` on the device -- must stay valid until smesh_synchronize or smesh_confusion_get.
 *
 * smesh_get_option("confusion_lds_max_classes", &v) (read-only) reports the class count up to which k_confusion keeps a
 * workgroup-private uint32 histogram in LDS (180: C (C + 1) + 1 counters in 128 KiB); beyond it samples are added straight into
 * the matrix in global memory.  "confusion_wave_aggregate" (0 / 1, default 1; smesh_set_option) turns the in-wave aggregation of
 * equal keys on and off (tools/confusion_bench.py measures both): same counts either way.
 */
#ifndef SMESH_EVAL_H
#define SMESH_EVAL_H

#include "smesh.h"
#include "smesh_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* smesh_profile_* slot of the counting kernel (smesh.h leaves slots 5 .. 7 free). */
#define SMESH_PROF_CONFUSION 5

typedef struct smesh_confusion smesh_confusion_t;

/* A zeroed matrix for C >= 1 classes in the memory of `device`.  C (C + 1) must stay below 2^31. */
int smesh_confusion_create(uint32_t C, int device, smesh_confusion_t** out);
int smesh_confusion_destroy(smesh_confusion_t* cm);
int smesh_confusion_reset(smesh_confusion_t* cm);
/* Waits for everything added so far; counts[C * (C + 1)] and *ignored in HOST memory (either may be NULL). */
int smesh_confusion_get(smesh_confusion_t* cm, uint64_t* counts, uint64_t* ignored);
/* Merges a HOST matrix of the same C (other ranks, scenes scored elsewhere). */
int smesh_confusion_add_counts(smesh_confusion_t* cm, const uint64_t* counts, uint64_t ignored);

/* Dense 1-D arrays: the per-vertex case.  pred: int32[n], gt: `gt_dtype`[n]. */
int smesh_confusion_add_labels(smesh_confusion_t* cm, const int32_t* pred, int pred_memkind,
                               const void* gt, int gt_dtype, int gt_memkind, uint64_t n);

/* int32 [P] labels of what smesh_aggregator_get would return, by the rule above; no [P, C] copy leaves the device.  Like get():
 * a pending row exchange is joined first, a reduce-scattered accumulator is refused.  Returns when `out` is complete. */
int smesh_aggregator_labels(smesh_aggregator_t* aggregator, float dont_care_threshold, int32_t* out, int memkind);

/* An index image that already exists (smesh_renderer_render output, a cache): the prediction of pixel (x, y) is
 * prim_labels[indices[x, y]].  `idx_dtype`: SMESH_IDX_*; P < 2^32 - 1 (the background value is never a primitive). */
int smesh_confusion_add_image(smesh_confusion_t* cm,
                              const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                              const int32_t* prim_labels, uint64_t P, int labels_memkind,
                              const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_memkind,
                              uint64_t W, uint64_t H);

/* Rasterise `camera` and score the view: the index plane never leaves HBM.  `prim_labels_dev`: int32[P] in DEVICE memory, P the
 * renderer's primitive count (triangles or texels alike); gt: (camera.width, camera.height). */
int smesh_confusion_add_view(smesh_confusion_t* cm, smesh_renderer_t* renderer, const smesh_camera_t* camera,
                             const int32_t* prim_labels_dev, uint64_t P,
                             const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_memkind);
/* `n` views; all ground-truth images share dtype, strides and memory.  Views are rasterised in groups of up to eight that share
 * their rasteriser launches, as in smesh_fuse_views. */
int smesh_confusion_add_views(smesh_confusion_t* cm, smesh_renderer_t* renderer, const smesh_camera_t* cameras, uint64_t n,
                              const int32_t* prim_labels_dev, uint64_t P,
                              const void* const* gts, int gt_dtype, const int64_t gt_strides[2], int gt_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_EVAL_H */
