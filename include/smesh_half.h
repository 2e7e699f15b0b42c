/*
 * smesh_half.h -- 16-bit class-vector images for libsmesh_hip.so: an extension of the C ABI in smesh.h.
 *
 * A segmentation network run under autocast outputs float16 or bfloat16.  The entry points below take such (W,H,C) images as they
 * are.  Each gives what its float32 counterpart in smesh.h gives for widen(image), where widen converts every element EXACTLY:
 *   float16:  IEEE binary16 -> binary32, subnormals included (a softmax output below 6.1e-5 is a float16 subnormal);
 *   bfloat16: the 16 bits become the upper half of the float32, the lower half is zero;
 *   +-0, +-inf and NaN map to themselves.
 * Everything after the widening is the specification of smesh.h: the `sum > 0.5f` test, the weights, the order of the additions and
 * the float32 accumulator.  Weights images stay float32.
 *
 * With a triangle renderer in the caller's face order, a Sum / Summax aggregator and at most "half_max_classes" classes a view is
 * fused by k_fuse_tri_h16, which reads the 16-bit rows in place (half the bytes of the float32 kernel's input).  Everything else --
 * Mul, texel renderers, re-ordered meshes, more classes, foreign index images, class stride != 1 -- gets the image widened ON THE
 * DEVICE into library scratch (k_widen_probs16) and takes the float32 path unchanged.  A HOST image crosses PCIe at 16 bits.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header; tests feed the oracle widen(image).
 *
 * smesh_last_fuse_kernel() (smesh.h) reports "k_fuse_tri_h16" after such a launch.  Two read-only names of smesh_get_option:
 * "half_max_classes" -- the largest class count k_fuse_tri_h16 serves (48) -- and "last_fuse_probs_dtype" -- the SMESH_PROBS_* code
 * of the class vectors that the calling thread's last fusion READ (0 when a widened image went through a float32 kernel).
 *
 * Conventions are those of smesh.h: images are (W,H,C) with the class fastest, strides in ELEMENTS and >= 0, every function returns
 * a status, SMESH_ERR_INVALID for a bad dtype, stride or shape.  SMESH_PROBS_F32 is refused by every entry point of this header:
 * callers with float32 images use smesh.h.
 */
#ifndef SMESH_HALF_H
#define SMESH_HALF_H

#include "smesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- class-vector dtypes ------------------------------------------------------------------- */
#define SMESH_PROBS_F32  0
#define SMESH_PROBS_F16  1
#define SMESH_PROBS_BF16 2

/* smesh_fuse_view (smesh.h) for a dense (W,H,C) image of `probs_dtype`; `weights`: dense float32 (W,H) in the same memory, or
 * NULL.  Asynchronous for DEVICE images (they must stay valid until smesh_synchronize / a completion token); HOST images are
 * consumed before the call returns. */
int smesh_fuse_view_probs16(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* camera,
                            const void* probs, int probs_dtype, const float* weights, int memkind);

/* smesh_fuse_views (smesh.h) for dense 16-bit images: `n` views in order, the same group pipeline, up to eight views per fusion
 * launch.  One dtype and one memory kind for the whole batch. */
int smesh_fuse_views_probs16(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                             const void* const* probs, int probs_dtype, const float* const* weights, int memkind);

/* smesh_aggregator_add (smesh.h) for a 16-bit image: any index image, any strided (W,H,C) image of `probs_dtype`.
 * `rendered_by_or_null`: the renderer whose latest smesh_renderer_render_device() output `indices` is, if the caller knows one --
 * that view takes the triangle-order kernel like smesh_fuse_view_probs16 (the library re-checks that it is the latest render; the
 * x and y strides of a network's (H,W,C) output seen as (W,H,C) are read in place); any other index image gets the class vectors
 * widened on the device and goes through smesh_aggregator_add_async.  Asynchronous for device images, like that function.
 * `idx_strides` / `weights_strides` NULL: dense; `probs_strides` NULL: dense. */
int smesh_aggregator_add_probs16(smesh_aggregator_t* aggregator, smesh_renderer_t* rendered_by_or_null,
                                 const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                                 const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_memkind,
                                 const float* weights, const int64_t weights_strides[2], int weights_memkind,
                                 uint64_t width, uint64_t height);

/* `n` float32 values rounded to `probs_dtype` (round to nearest, ties to even; overflow gives inf, subnormal results are kept, NaN
 * stays NaN) on GPU `device`.  `in` and `out` (2 * n bytes) are both in `memkind` memory; asynchronous for DEVICE memory.  For
 * tests, benchmarks and callers whose network ran in float32. */
int smesh_narrow_probs(const float* in, void* out, uint64_t n, int probs_dtype, int device, int memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_HALF_H */
