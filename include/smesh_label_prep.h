/*
 * smesh_label_prep.h -- label images at their OWN resolution and in the DATASET's ids: an extension of smesh_labels.h.
 *
 * Two things every real mask needs before it can be fused or scored, and which the reference's scripts do per frame on the host:
 * the ground truth of eval-scannet/eval_scannet.py:232-234 / :311-313 goes through tf.gather(scannet_to_nyu40, gt) -- raw dataset
 * ids, a table of about 1 360 entries, to 40 classes, -1 for "unmapped" --, and a mask that comes from a network is at the network's
 * resolution, not the camera's.  The entry points below take the (w,h) image and the table as they are and build the dense (W,H)
 * plane of smesh_labels.h on the device, in one kernel (k_labels_prepare, csrc/label_prep.hip).
 *
 * THE RULE, to the bit.
 *   Sampling: nearest neighbour with half-pixel centres, in integers.  Per axis, with source size n, target size N and target
 *   coordinate X in [0, N):
 *       i = ((2X + 1) * n) div (2N)
 *   the exact floor of (X + 0.5) * n / N.  i < n always (no clamp); n == N is the identity; (2X + 1) * n comes to just
 *   under 2^33 at the size limits, so the product is formed in 64 bits.  No floating point takes part.  This is what TF2's
 *   tf.image.resize(method="nearest"), torch's mode="nearest-exact" and PIL compute; it is NOT torch's legacy mode="nearest",
 *   which is floor(X * n / N).
 *   Map: `map` is int32 [map_len].  A source value v with 0 <= v < map_len becomes map[v]; every other v, negative ones included,
 *   is don't care.  Without a map v stays v.
 *   Order: sample first, then map.
 *   Narrowing, unchanged from smesh_labels.h / smesh_eval.h: a value outside [0, C) after the map (or without one) becomes the
 *   all-ones code of the plane -- 255 in a uint8 plane (C <= 255), 65535 in a uint16 plane.  Such a pixel adds nothing but still
 *   counts as a pixel of its primitive; as ground truth it enters no cell and counts as ignored.
 *
 * The kernel: one lane per output pixel, lanes along the output's y, every layout and ratio.  A map of at most
 * SMESH_LABEL_PREP_MAP_LDS_MAX entries is copied into LDS once per workgroup, as narrowed 2-byte codes; a longer one is gathered
 * from global memory.  (A second, tiled form for sources whose fastest axis is x, with its option "labels_prepare_tiles", was
 * measured and removed: it did not beat this one beyond the spread of the measurement)  Read-only:
 * smesh_get_option("labels_prepare_map_lds_max") reports the limit, "labels_prepare_launches" counts the launches of the kernel in
 * this process.
 *
 * PRODUCT-ONLY, like smesh_labels.h: the oracle implements nothing of this header.
 *
 * Refused with SMESH_ERR_INVALID and a message, before anything is changed: w == 0 or h == 0 with a non-empty target; w, h, W or H
 * over 65536, or W * H >= 2^29; map_len == 0 with a non-NULL map, map_len != 0 with a NULL one, or map_len > 2^24; a bad dtype or
 * memory kind; negative strides; more than 65535 classes (more than 255 for a uint8 output plane).
 *
 * Conventions are those of smesh_labels.h: images are (width, height) with y fastest, strides in ELEMENTS and >= 0 (NULL: dense).
 */
#ifndef SMESH_LABEL_PREP_H
#define SMESH_LABEL_PREP_H

#include "smesh_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest map that k_labels_prepare copies into LDS (2 bytes an entry: 8 KiB of a workgroup's 64 KiB; no more entries than a
 * workgroup has output pixels, so the copy never outweighs the work it serves). */
#define SMESH_LABEL_PREP_MAP_LDS_MAX 4096

/* The dense (W,H) plane of a (w,h) label image: `in` of `label_dtype` (SMESH_LBL_*) at element strides `in_strides` in `in_memkind`
 * memory; `map_or_null` int32 [map_len] in `map_memkind` memory; C classes.  `out`: DEVICE memory on `device`, W * H elements of
 * `out_dtype` (SMESH_LBL_U8, which needs C <= 255, or SMESH_LBL_U16).  A host source is staged at its own size and span: w * h
 * elements cross PCIe, not W * H.  Returns when the plane is written. */
int smesh_labels_prepare(const void* in, int label_dtype, const int64_t in_strides[2], int in_memkind, uint64_t w, uint64_t h,
                         const int32_t* map_or_null, uint64_t map_len, int map_memkind, uint32_t C,
                         void* out, int out_dtype, uint64_t W, uint64_t H, int device);

/* smesh_fuse_views_labels / smesh_fuse_view_labels / smesh_aggregator_add_labels (smesh_labels.h) for label images of (w,h) pixels
 * and an optional map: each image is prepared into the plane scratch of its group of eight (never used in place), host images are
 * staged at their own size, the map is staged once per call, and from there on the call is its counterpart's -- the same kernels,
 * the same routes.  One (w,h), one dtype, one set of strides and one map per call; each camera keeps its own (W,H); weights images
 * stay (W,H). */
int smesh_fuse_views_labels_prepared(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                     const void* const* labels, int label_dtype, const int64_t label_strides[2],
                                     const float* const* weights, int memkind,
                                     uint64_t w, uint64_t h, const int32_t* map_or_null, uint64_t map_len, int map_memkind);

int smesh_fuse_view_labels_prepared(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* camera,
                                    const void* labels, int label_dtype, const int64_t label_strides[2],
                                    const float* weights, int memkind,
                                    uint64_t w, uint64_t h, const int32_t* map_or_null, uint64_t map_len, int map_memkind);

int smesh_aggregator_add_labels_prepared(smesh_aggregator_t* aggregator, smesh_renderer_t* rendered_by_or_null,
                                         const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                                         const void* labels, int label_dtype, const int64_t label_strides[2], int label_memkind,
                                         const float* weights, const int64_t weights_strides[2], int weights_memkind,
                                         uint64_t width, uint64_t height,
                                         uint64_t w, uint64_t h, const int32_t* map_or_null, uint64_t map_len, int map_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_LABEL_PREP_H */
