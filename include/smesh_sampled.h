/*
 * smesh_sampled.h -- class-vector images at the network's resolution fused into views at the camera's, sampled inside the fusion
 * kernel: an extension of the C ABI in smesh.h.
 *
 * smesh_resize.h resamples a (w,h,C) image to the dense (W,H,C) image the fusion kernels read; the fusion then reads only the visible
 * pixels of each triangle from it.  The entry points below fuse the (w,h,C) image as it is: for a visible pixel (X,Y) of a view the
 * kernel computes the class vector from the four source rows around it, by the rule of smesh_resize.h, and adds it.
 * No (W,H,C) image is written, read back or allocated.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * Results are those of smesh_resize_probs with out_dtype = probs_dtype followed by the entry point of smesh.h /
 * smesh_half.h for that dtype, to the bit where that entry point is bit-exact: the blended float32 row of a float16 / bfloat16 source is
 * rounded to the source's dtype (the rule of smesh_narrow_probs) and widened again before the `sum > 0.5f` test and the additions,
 * because that is what the resampled image holds.
 *
 * Conventions are those of smesh_resize.h and smesh_half.h: class-vector images are (w,h,C) with C the aggregator's class count;
 * strides are in ELEMENTS and >= 0, NULL means dense (class fastest, then y); `probs_dtype` is SMESH_PROBS_F32 | F16 | BF16; `mode` is
 * SMESH_RESIZE_BILINEAR; weights images are float32 at the VIEW's size (W,H).  SMESH_ERR_INVALID comes with a message
 * (smesh_last_error) and leaves nothing changed.  Refused: w == 0 or h == 0, w or h over 65536, a bad dtype or mode, an image that is
 * not aligned to its element size.  HOST images are staged at the source's size, at most eight at a time, and consumed before the
 * call returns; DEVICE images are read asynchronously in place and must stay valid until smesh_synchronize / a completion token.
 *
 * Routes.  k_fuse_tri_sampled serves a view of a triangle renderer in the caller's face order into a Sum or Summax aggregator of
 * at most 48 classes, from an image with class stride 1 -- dense, or a network's (h,w,C) tensor seen as (w,h,C) with strides
 * (C, w C, 1) -- and, for smesh_aggregator_add_sampled, an index plane that is the renderer's own latest render.  Everything else
 * (Mul, texel renderers, re-ordered meshes, C > 48, a class stride other than 1 such as a channel-first tensor, foreign index images)
 * is resampled by smesh_resize_probs into scratch of the aggregator inside the call, at most eight images at a time, and takes the
 * existing entry point.  A call whose images have the views' size already and are dense passes them through untouched to that
 * entry point.  After a launch of the kernel smesh_last_fuse_kernel() is "k_fuse_tri_sampled" and the read-only options
 * "last_fuse_slot" / "last_fuse_views" give the instance (register slots 8 .. 48, views 1 / 2 / 4 / 8).
 * smesh_set_option("fuse_sampled", 0 | 1) (default 1; the environment's SMESH_FUSE_SAMPLED=0 sets the default) is a test hook: 0 sends
 * every call of these entry points down the resample-then-fuse route.
 */
#ifndef SMESH_SAMPLED_H
#define SMESH_SAMPLED_H

#include "smesh.h"
#include "smesh_half.h"
#include "smesh_resize.h"

#ifdef __cplusplus
extern "C" {
#endif

/* smesh_fuse_views (smesh.h) for `n` views whose class vectors are (w,h,C) images: one dtype, one set of strides and one (w,h) for the
 * whole call, each camera with its own (W,H).  The group pipeline and the eight-views-per-launch grouping are smesh_fuse_views'.
 * `weights`: NULL, or one dense float32 (W,H) image per view in the same memory as the class vectors. */
int smesh_fuse_views_sampled(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                             const void* const* probs, int probs_dtype, const int64_t probs_strides[3], uint64_t w, uint64_t h,
                             const float* const* weights, int memkind, int mode);

/* One view of it. */
int smesh_fuse_view_sampled(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* camera,
                            const void* probs, int probs_dtype, const int64_t probs_strides[3], uint64_t w, uint64_t h,
                            const float* weights, int memkind, int mode);

/* smesh_aggregator_add (smesh.h) for a (w,h,C) image and a (W,H) index image, in the shape of smesh_aggregator_add_probs16:
 * `rendered_by_or_null` is the renderer whose latest smesh_renderer_render_device() output `indices` is, if the caller knows one (the
 * library re-checks it).  One library call and one fusion launch per view. */
int smesh_aggregator_add_sampled(smesh_aggregator_t* aggregator, smesh_renderer_t* rendered_by_or_null,
                                 const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                                 const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_memkind,
                                 const float* weights, const int64_t weights_strides[2], int weights_memkind,
                                 uint64_t w, uint64_t h, uint64_t W, uint64_t H, int mode);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_SAMPLED_H */
