/*
 * smesh_labels.h -- label-image entry points of libsmesh_hip.so: an extension of the C ABI in smesh.h.
 *
 * The reference's user script fuses MASK images -- one class index per pixel -- and has to blow each of them up to a one-hot
 * (W,H,C) float32 tensor because its aggregator takes nothing else (python/scripts/colorize_mesh.py:39-67,
 * eval-scannet/eval_scannet.py:232-234).  The entry points below take the mask itself.  Each gives what its class-vector
 * counterpart in smesh.h gives for one_hot(labels), where one_hot is tf.one_hot: a label outside [0, C), negative values
 * included, is the all-zero "don't care" vector (such a pixel adds nothing but still counts as a pixel of its primitive).
 * Stated for finite weights: with a non-finite weight the one-hot path computes 0 * inf = NaN for the other classes of the
 * pixel, which these entry points do not reproduce.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header; tests feed the oracle one-hot vectors.
 *
 * smesh_get_option("labels_lds_max_classes", &v) (smesh.h; read-only, smesh_set_option refuses it) reports the class count up to
 * which k_fuse_tri_labels keeps a wave's 64 accumulator rows in LDS (255); beyond it the owner lane read-modify-writes the row
 * in global memory.
 *
 * Two more read-only names report which instance of the triangle-order fusion the calling thread's last launch was (class vectors,
 * not labels; smesh_last_fuse_kernel names the kernel from the class count alone): "last_fuse_slot" is the class-count slot handed
 * to k_fuse_tri -- 5, 13, 19, 20, 21, 40 for the exact instances, 8, 16, 24, 32, 41, 48 for the run-time-C instances with 8, 16, 24,
 * 32, 40 and 48 register slots --, 0 when the launch was k_fuse_tri_any, k_fuse_tri_wide or k_fuse_tri_wide_list, -1 before the
 * first such launch; "last_fuse_views" is the number of views of that launch (1, 2, 4 or 8).  For a k_fuse_tri_labels launch
 * "last_fuse_slot" is 0, "last_fuse_views" its views, and the read-only "last_fuse_labels_form" reports the rest of the instance: the
 * bytes per label of the planes it read (1: uint8, 2: uint16), plus 16 where the rows were kept in LDS; 0 before the first launch.
 * "last_fuse_flagged_views" (read-only; also for k_fuse_tri_h16 and k_fuse_tri_sampled): bit v is set when view v of that launch had
 * its "check the masks against the index plane" flag up (fragment-queue overflow, direct rasteriser).  It is read back from the
 * device when asked -- the call waits for the device -- and reads 0 once any renderer has been destroyed since that launch.
 * "compute_units" (read-only): the compute units of device 0 as the library sizes launches by them (these kernels' tail blocks:
 * 16 per unit).
 *
 * Conventions are those of smesh.h: label images are (W,H) with y fastest, strides in ELEMENTS and >= 0, every function
 * returns a status, SMESH_ERR_INVALID for a bad dtype, stride or shape.
 */
#ifndef SMESH_LABELS_H
#define SMESH_LABELS_H

#include "smesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- label dtypes -------------------------------------------------------------------------- */
#define SMESH_LBL_U8  0
#define SMESH_LBL_I8  1
#define SMESH_LBL_U16 2
#define SMESH_LBL_I16 3
#define SMESH_LBL_U32 4
#define SMESH_LBL_I32 5
#define SMESH_LBL_U64 6
#define SMESH_LBL_I64 7

/* smesh_fuse_view (smesh.h) for a label image: render `camera` and add one_hot(labels).  `labels`: (W,H) of `label_dtype` at
 * element strides `label_strides` (NULL: dense); `weights`: dense float32 (W,H) in the same memory, or NULL.  With a triangle
 * renderer in the caller's face order and a Sum / Summax aggregator the view is fused by k_fuse_tri_labels (one addition per
 * visible pixel, no class vector is ever built); everything else expands the labels ON THE DEVICE and takes smesh_fuse_view's
 * path.  Asynchronous for DEVICE images (they must stay valid until smesh_synchronize / a completion token); HOST images are
 * consumed before the call returns, and only the narrow (one or two bytes per pixel) plane crosses PCIe. */
int smesh_fuse_view_labels(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* camera,
                           const void* labels, int label_dtype, const int64_t label_strides[2],
                           const float* weights, int memkind);

/* smesh_fuse_views (smesh.h) for label images: `n` views in order, the same group pipeline, up to eight views per fusion
 * launch (each accumulator row makes one round trip for all of them).  All label images share dtype, strides and memory. */
int smesh_fuse_views_labels(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                            const void* const* labels, int label_dtype, const int64_t label_strides[2],
                            const float* const* weights, int memkind);

/* smesh_aggregator_add (smesh.h) for a label image: any index image, any label image.  `rendered_by_or_null`: the renderer
 * whose latest smesh_renderer_render_device() output `indices` is, if the caller knows one -- that view takes the
 * triangle-order label kernel like smesh_fuse_view_labels (the library re-checks that it is the latest render); any other
 * index image gets the labels expanded on the device and goes through smesh_aggregator_add_async.
 * `idx_strides` / `label_strides` / `weights_strides` NULL: dense. */
int smesh_aggregator_add_labels(smesh_aggregator_t* aggregator, smesh_renderer_t* rendered_by_or_null,
                                const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_memkind,
                                const void* labels, int label_dtype, const int64_t label_strides[2], int label_memkind,
                                const float* weights, const int64_t weights_strides[2], int weights_memkind,
                                uint64_t width, uint64_t height);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_LABELS_H */
