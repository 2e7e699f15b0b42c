/*
 * smesh_label_colors.h -- label images that are COLOUR images: an extension of smesh_label_prep.h.
 *
 * Cityscapes *_color.png, ADE20K, VOC palette PNGs and most labelling tools export a mask as an (H,W,3) uint8 image in which each
 * class is a colour.  The reference's colorize_mesh.py --remap (lines 44-56) turns such a mask into class indices per frame on the
 * host: np.unique over the rows of the image, a dictionary colour -> class that grows as new colours appear, an index image, then
 * tf.one_hot.  The entry points below do both halves on the device: the distinct colours of images (smesh_colors_unique: what the
 * dictionary is grown from), and the dense (W,H) plane of smesh_labels.h from a colour image and a colour table
 * (k_labels_prepare_colors, csrc/label_colors.hip), alone or in front of the label fusion.  The inverse direction -- the fused mesh
 * rendered into colour images -- is smesh_label_images.h.
 *
 * THE RULE, to the bit.
 *   Image: (w, h, ch) uint8 with ch = 3 or 4 and three non-negative ELEMENT strides (NULL: dense, h * ch, ch, 1).  A decoded
 *   (H,W,3) array is handed over as its transposed (1,0,2) view: strides (3, 3 W, 1).  Channels 0, 1, 2 are r, g, b.  A fourth
 *   channel (alpha) is read by nobody and is no part of the key.
 *   Key: key = r << 16 | g << 8 | b, an integer in [0, 2^24).  Ascending key order is the lexicographic order of (r, g, b) rows:
 *   the order of np.unique(rows, axis=0).
 *   Colour table: K pairs (keys[j], classes[j]) in HOST memory, 1 <= K <= 2^24, keys uint32 and STRICTLY ascending (so below 2^24
 *   and without repeats), classes int32.  It is staged once per call, like the map of smesh_label_prep.h.
 *   Lookup: a pixel whose key is keys[j] gets classes[j]; a key that is not in the table is don't care.
 *   Narrowing, unchanged from smesh_labels.h: a class outside [0, C) becomes the all-ones code of the plane (255 in a uint8 plane,
 *   which needs C <= 255; 65535 in a uint16 plane).
 *   Sampling: the rule of smesh_label_prep.h, i = ((2X + 1) * n) div (2N) per axis, in integers.  Sample first, then look up.
 *   Distinct colours of an image: the ascending list of the keys that occur in it.  Here a 2-D image is accepted too (ch = 1, uint8
 *   or uint16, key = value): the script's color_channels == 1 case.
 *
 * The kernels.  k_colors_mark sets bit `key` of a bitmap of 2^24 bits (2 MiB an image, one bitmap per image of a group of eight,
 * cleared by one memset per group); a lane whose left neighbour in the wave holds the same key leaves the test to it, the others
 * test their bit with a plain load and issue the atomic OR only where it reads 0.
 * k_colors_count / k_colors_list turn a bitmap into the ascending key list by population counts and a prefix sum over its words: no
 * pixel is sorted, and the bitmap is left intact.  k_labels_prepare_colors has k_labels_prepare's structure -- one lane per output
 * pixel, lanes along the output's y, 4096 pixels per workgroup of 256 --; a table of at most SMESH_LABEL_COLORS_LDS_MAX entries is
 * copied into LDS once per workgroup (4-byte keys, 2-byte narrowed codes) and bisected there, a longer one is bisected in global
 * memory.  Plain loads and stores, no atomics, no floating point.  Read-only: smesh_get_option("labels_colors_lds_max") reports the
 * limit, "labels_colors_launches" counts the launches of k_labels_prepare_colors in this process (k_labels_prepare's own counter,
 * "labels_prepare_launches", does not move for a colour image).
 *
 * PRODUCT-ONLY, like smesh_labels.h: the oracle implements nothing of this header.
 *
 * Refused with SMESH_ERR_INVALID and a message, before anything is changed: a channel count other than 3 or 4 (1 is accepted by
 * smesh_colors_unique only); a dtype other than uint8 (uint16 too for one channel); negative strides; K == 0, K > 2^24 or a NULL
 * table; keys that are not strictly ascending or a key >= 2^24; the size limits of smesh_label_prep.h (an empty source with a
 * non-empty target; w, h, W or H over 65536; W * H >= 2^29); a bad memory kind; more than 65535 classes (more than 255 for a uint8
 * output plane).
 *
 * Conventions are those of smesh_labels.h: images are (width, height[, channel]), strides in ELEMENTS and >= 0.
 */
#ifndef SMESH_LABEL_COLORS_H
#define SMESH_LABEL_COLORS_H

#include "smesh_label_prep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest colour table that k_labels_prepare_colors copies into LDS: 4-byte keys and 2-byte narrowed codes, 24 KiB of the 64 KiB a
 * workgroup gets without asking; no more entries than a workgroup has output pixels. */
#define SMESH_LABEL_COLORS_LDS_MAX 4096

/* The distinct colours of `n` images of one shape (w, h, channels), one `dtype` (SMESH_LBL_U8; SMESH_LBL_U16 too with channels == 1),
 * one set of `strides` (three; the third is ignored with channels == 1) and one memory kind.  keys_out: HOST uint32 [n][cap], row i
 * the ascending keys of image i, at most `cap` of them (cap == 0: keys_out may be NULL); counts_out: HOST uint64 [n], the TRUE
 * number of distinct keys of each image even where it exceeds `cap` -- a caller whose rows were too short asks again.  The images are
 * worked off in groups of eight with one synchronisation per group; host images are staged at their own span. */
int smesh_colors_unique(const void* const* images, uint64_t n, int channels, int dtype, const int64_t strides[3], int memkind,
                        uint64_t w, uint64_t h, uint32_t* keys_out, uint64_t cap, uint64_t* counts_out, int device);

/* smesh_labels_prepare for a colour image and a colour table: `in` uint8 (w, h, channels) at `in_strides` in `in_memkind` memory;
 * the table in HOST memory; `out`: DEVICE memory on `device`, W * H elements of `out_dtype` (SMESH_LBL_U8, which needs C <= 255, or
 * SMESH_LBL_U16).  Returns when the plane is written. */
int smesh_labels_prepare_colors(const void* in, int channels, const int64_t in_strides[3], int in_memkind, uint64_t w, uint64_t h,
                                const uint32_t* keys, const int32_t* classes, uint64_t K, uint32_t C,
                                void* out, int out_dtype, uint64_t W, uint64_t H, int device);

/* smesh_fuse_views_labels_prepared / smesh_fuse_view_labels_prepared / smesh_aggregator_add_labels_prepared (smesh_label_prep.h) for
 * colour images of (w, h, channels) and a colour table in place of the map: each image is prepared into the plane scratch of its
 * group of eight, host images are staged at their own span, the table is staged once per call, and from there on the call is its
 * counterpart's -- the same kernels, the same routes.  `label_dtype` is SMESH_LBL_U8, `label_strides` has THREE entries.  One shape,
 * one set of strides and one table per call; each camera keeps its own (W,H); weights images stay (W,H). */
int smesh_fuse_views_labels_colors(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                   const void* const* labels, int label_dtype, const int64_t label_strides[3],
                                   const float* const* weights, int memkind,
                                   uint64_t w, uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K);

int smesh_fuse_view_labels_colors(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* camera,
                                  const void* labels, int label_dtype, const int64_t label_strides[3],
                                  const float* weights, int memkind,
                                  uint64_t w, uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K);

int smesh_aggregator_add_labels_colors(smesh_aggregator_t* aggregator, smesh_renderer_t* rendered_by_or_null,
                                       const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                                       const void* labels, int label_dtype, const int64_t label_strides[3], int label_memkind,
                                       const float* weights, const int64_t weights_strides[2], int weights_memkind,
                                       uint64_t width, uint64_t height,
                                       uint64_t w, uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_LABEL_COLORS_H */
