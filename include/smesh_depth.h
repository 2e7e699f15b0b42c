/*
 * smesh_depth.h -- fusion gated by SENSOR DEPTH: consistency weights computed on the device, an extension of smesh.h.
 *
 * Every fusion call assumes that the pixel a face projects to really shows that face.  Where the camera saw something that is not in
 * the mesh (or saw through geometry that is), the network's class for that pixel is added to the wrong face.  RGB-D datasets ship the
 * cure with every frame (eval-scannet/eval_scannet.py:219 decodes frame.decompress_depth_zlib()): compare the sensor's depth with the
 * rendered depth and drop the pixels that disagree.  The entry points below compute the weights image that does so -- the plane that
 * every fusion kernel already multiplies into a pixel's contribution -- in one kernel (k_depth_weights, csrc/depth_weights.hip)
 * between the rasteriser and the fusion launch, for up to eight views per launch.
 *
 * THE RULE, to the bit.  A gate is five numbers: scale, abs_tol, rel_tol, max_depth (+inf: none), missing_keep (0 / 1).  For output
 * pixel (X, Y) of the camera's (W, H), every operation a single float32 IEEE operation, in this order, never fused:
 *   d_r   the rendered depth at (X, Y): float32, +inf for background (smesh_renderer_render).
 *   raw   the sensor image at (x, y), x = ((2X + 1) w) div (2W), y likewise: the nearest-neighbour rule of smesh_label_prep.h, the same
 *         code (csrc/nearest_rule.hpp); (w, h) == (W, H) is the identity.
 *   d_s   = float(raw) * scale.   A uint16 sample is MISSING when raw == 0, a float32 sample when !(raw > 0) or it is not finite.
 *   t     = abs_tol + rel_tol * d_s        (a multiply, then an add)
 *   diff  = |d_r - d_s|
 *   1. d_r not finite      -> background,    weight 0
 *   2. d_r > max_depth     -> far,           weight 0
 *   3. the sample missing  -> missing,       weight missing_keep ? w_in : 0
 *   4. !(diff <= t)        -> inconsistent,  weight 0
 *   5. otherwise                              weight w_in
 *   w_in is the caller's weights image at (X, Y), or 1.0f.
 * Counts per view: uint64 [visible, far, missing, inconsistent]; visible = d_r finite; a pixel is in at most one of the other three
 * (a far pixel with a missing sample counts as far).
 *
 * The kernel: one lane per output pixel, lanes along the output's y, every source layout and ratio; the dense depth and weights
 * planes move in 16 bytes per lane where the planes are 16-byte aligned, the last W * H mod 4 pixels one by one; the view comes from
 * the block index, so ONE launch serves a group of up to eight views; a workgroup takes 4096 consecutive pixels, and the XCDs take
 * the workgroups in runs, so that a line of a transposed source is fetched into one L2.  Counts: ballot and population
 * count per wave, one atomic add per wave and counter.  Measured on an MI355X, eight views per launch: 55 us for 640 x 480 uint16 ->
 * 1296 x 968, 107 us for 1920 x 1080 float32 at full size -- a fifth of what 8 TB/s would allow: bound by latency.
 * Read-only: smesh_get_option("depth_weights_launches") counts the launches of the kernel in this process.
 *
 * PRODUCT-ONLY: the oracle implements nothing of this header.
 *
 * Refused with SMESH_ERR_INVALID and a message, before anything is changed: w == 0 or h == 0; w, h, W or H over 65536; negative
 * strides; a bad dtype, image kind or memory kind; a NaN or negative scale, abs_tol or rel_tol; a NaN max_depth.
 *
 * Conventions are those of smesh.h: images are (width, height) with y fastest, strides in ELEMENTS and >= 0 (NULL: dense).
 */
#ifndef SMESH_DEPTH_H
#define SMESH_DEPTH_H

#include "smesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sensor depth dtypes */
#define SMESH_DEPTH_U16 0
#define SMESH_DEPTH_F32 1

/* what the images of smesh_fuse_views_depth are: dense (W,H,C) class vectors of float32 / float16 / bfloat16 (the SMESH_PROBS_*
 * codes of smesh_half.h), or dense (W,H) label planes of uint8 / uint16 (smesh_labels.h: a value >= C is don't care) */
#define SMESH_DEPTH_IMG_F32       0
#define SMESH_DEPTH_IMG_F16       1
#define SMESH_DEPTH_IMG_BF16      2
#define SMESH_DEPTH_IMG_LABELS_U8  3
#define SMESH_DEPTH_IMG_LABELS_U16 4

typedef struct smesh_depth_gate {
  float   scale;         /* sensor units -> the mesh's units (ScanNet's millimetres: 0.001f) */
  float   abs_tol;
  float   rel_tol;
  float   max_depth;     /* +inf: none */
  int32_t missing_keep;  /* 0 / 1 */
} smesh_depth_gate_t;

/* The weights plane of ONE view.  `depth`: dense float32 (W,H) in DEVICE memory on `device` (smesh_renderer_render_device's plane);
 * `sensor`: (w,h) of `sensor_dtype` at element strides `sensor_strides` in `sensor_memkind` memory -- a host image is staged at its
 * own size and span; `weights_in_or_null`: dense float32 (W,H) in DEVICE memory; `weights_out`: DEVICE memory, W * H floats (it may be
 * `weights_in_or_null`).  `counts_or_null`: HOST uint64 [4]; asking for counts makes the call wait for them, without them the call
 * returns when the kernel is queued behind everything the library has queued so far (a host sensor: when it has been staged). */
int smesh_depth_weights(const float* depth, uint64_t W, uint64_t H,
                        const void* sensor, int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind, uint64_t w, uint64_t h,
                        const smesh_depth_gate_t* gate, const float* weights_in_or_null, float* weights_out,
                        uint64_t* counts_or_null, int device);

/* smesh_fuse_views (smesh_fuse_views_probs16 / smesh_fuse_views_labels for the other image kinds) with every view gated by its
 * sensor image.  `images`: n dense images of `image_kind` at each camera's resolution, in DEVICE memory; `weights_or_null`: NULL or n
 * dense float32 (W,H) planes in DEVICE memory (single entries may be NULL), multiplied in as w_in; `sensors`: n (w,h) images of one
 * dtype, one set of strides and one memory kind; each camera keeps its own (W,H).  `counts_or_null`: HOST uint64 [n][4]; asking for
 * them makes the call wait.
 * Per group of up to eight views: the views are rasterised with their depth planes, ONE k_depth_weights launch writes their weights
 * planes (library-owned), and the group's ordinary fusion launch reads those planes as its weights.  Where the k_fuse_tri family
 * serves the renderer and the aggregator the group is fused by the launches of the plain call (smesh_last_fuse_kernel reports the
 * same kernel); everything else -- texel renderers, class counts beyond the family's, Mul where it has no group kernel -- is fused
 * view by view from the same planes.  The sums are those of the plain call with the rule's weights images, in its order. */
int smesh_fuse_views_depth(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                           const void* const* images, int image_kind, const float* const* weights_or_null,
                           const void* const* sensors, int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind,
                           uint64_t w, uint64_t h, const smesh_depth_gate_t* gate, uint64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_DEPTH_H */
