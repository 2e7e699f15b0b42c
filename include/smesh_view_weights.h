/*
 * smesh_view_weights.h -- fusion weighted by VIEWING GEOMETRY: incidence-angle and distance weights computed on the device, an
 * extension of smesh.h with the shape of smesh_depth.h.
 *
 * Every fusion call treats a pixel as equally good evidence for the face it lands on, however the face was seen.  A face seen at 85
 * degrees from its normal, or from far away, covers a handful of pixels along its silhouette: there a network's prediction is least
 * reliable and a small pose error moves the projection onto a neighbour.  The standard cure in multi-view semantic fusion is to weight a
 * pixel by the cosine of its incidence angle, often with a falloff in distance.  The weight needs what the library holds after
 * rasterising and the caller does not: the index plane and the depth plane of THAT render and the mesh's face normals.  The entry
 * points below compute the weights image -- the plane every fusion kernel already multiplies into a pixel's contribution -- in one
 * kernel (k_view_weights, csrc/view_weights.hip) between the rasteriser and the fusion launch, for up to eight views per launch.
 *
 * THE RULE, to the bit.  Every operation is a single IEEE operation in the stated order, never fused.
 *
 * Face normals: one per triangle (v0, v1, v2), float32:  e1 = v1 - v0,  e2 = v2 - v0,  n = e1 x e2, each component two multiplies and
 * one subtract (nx = e1y*e2z - e1z*e2y,  ny = e1z*e2x - e1x*e2z,  nz = e1x*e2y - e1y*e2x); not normalised.  A face with a vertex index
 * outside [0, V) has the normal (0, 0, 0).  The table is built once per renderer on the device at first use, kept with it, and indexed
 * by the id the index plane holds -- the caller's face id, also where the renderer processes the mesh in another order.
 *
 * A spec is five numbers and an optional plane: power (integer, 0 .. SMESH_VW_MAX_POWER), min_cos (in [0, 1]), two_sided (0 / 1),
 * max_depth (+inf: none), falloff_depth (+inf: none, else > 0), and the weights-in plane.
 *
 * Per output pixel (X, Y) of a camera (W, H), id from the index plane, d_r from the depth plane, F the renderer's face count:
 *   1. d_r not finite, id == 0xFFFFFFFF or id >= F  -> background,  weight 0
 *   2. d_r > max_depth                               -> far,         weight 0
 *   3. the pixel's ray in camera coordinates and the cosine:
 *        a = ((X + 0.5) - cx) / fx,  b = ((Y + 0.5) - cy) / fy     in double from the camera's double focal / principal, each
 *                                                                    rounded to float32 (the pixel centre of the rasteriser)
 *        n_c = R n   in float32, left to right:  n_cx = (R00*nx + R01*ny) + R02*nz, ...
 *        dot = (n_cx*a + n_cy*b) + n_cz
 *        nn  = (n_cx*n_cx + n_cy*n_cy) + n_cz*n_cz
 *        dd  = (a*a + b*b) + 1.0f
 *        c   = |dot| / sqrtf(nn * dd);   c = 0 when !(nn > 0) or nn * dd is not finite (a degenerate face)
 *   4. two_sided == 0 and dot > 0 (the face looks away from the camera)  -> backfacing,  weight 0
 *   5. !(c >= min_cos)                               -> grazing,     weight 0   (a degenerate face counts here when min_cos > 0)
 *   6. otherwise:  g = 1.0f, then `power` times g = g * c;
 *                  f = 1.0f; with a falloff  q = d_r / falloff_depth,  f = 1.0f / (1.0f + q*q);
 *                  weight = (w_in * g) * f,   w_in the caller's weights image at (X, Y), or 1.0f.
 * Counts per view: uint64 [visible, far, grazing, backfacing]; visible = the pixels that pass step 1; a pixel is in at most one of
 * the other three.  With power 0, min_cos 0, two_sided 1, no max_depth and no falloff the weight is w_in in bits for every
 * non-background pixel.
 *
 * sqrtf and the two float32 divisions are the correctly rounded ones: the library is compiled without -ffast-math and with the
 * compiler's default -fhip-fp32-correctly-rounded-divide-sqrt, under which the device's sqrtf and / are correctly rounded and keep
 * subnormals; tests/view_weights_ref.py (numpy, which is) decides.  powf is not used, which is why `power` is an integer.
 *
 * The kernel: one lane per output pixel, lanes along the output's y, four consecutive pixels per lane per round; the index, depth and
 * weights planes move in 16 bytes per lane where they are 16-byte aligned, the last W * H mod 4 pixels and unaligned planes one by
 * one; the view comes from the block index, so ONE launch serves a group of up to eight views, each with its own (W, H) and camera
 * (the cameras travel in the kernel's arguments); a workgroup takes 4096 consecutive pixels, and the XCDs take the workgroups in
 * runs.  The normals table holds one 16-byte element per face -- one load per pixel, mostly of a line a neighbour already fetched.
 * Counts: ballot and population count per wave, one atomic add per wave and counter.  Measured on an MI355X, eight views per launch: 72 us at 1296 x 968, 108 us at 1920 x 1080 --
 * a fifth of what 8 TB/s would allow for the planes, 1.9 times k_depth_weights: bound by its arithmetic.
 * Read-only: smesh_get_option("view_weights_launches") counts the launches in this process.
 *
 * PRODUCT-ONLY: the oracle implements nothing of this header.
 *
 * Refused with SMESH_ERR_INVALID and a message, before anything is changed: everything smesh_depth.h refuses about planes, sizes,
 * sensor images and gates; power outside 0 .. 16; min_cos NaN or outside [0, 1]; a NaN max_depth; falloff_depth NaN or <= 0; a
 * TEXEL renderer -- its index plane holds texel ids, and a texel -> face lookup is not built.
 */
#ifndef SMESH_VIEW_WEIGHTS_H
#define SMESH_VIEW_WEIGHTS_H

#include "smesh.h"
#include "smesh_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMESH_VW_MAX_POWER 16

typedef struct smesh_view_weights_spec {
  int32_t power;          /* 0 .. SMESH_VW_MAX_POWER: the weight is cos^power */
  float   min_cos;        /* [0, 1]: a pixel seen at a smaller cosine gets weight 0 */
  int32_t two_sided;      /* 0: a face that looks away from the camera gets weight 0;  1: |cos| */
  float   max_depth;      /* +inf: none */
  float   falloff_depth;  /* +inf: none; else > 0: the weight is divided by 1 + (d_r / falloff_depth)^2 */
} smesh_view_weights_spec_t;

/* The weights plane of ONE view.  `indices_dev`, `depth_dev`: the dense uint32 / float32 (W,H) planes of
 * smesh_renderer_render_device(renderer, camera) (or copies of them) in DEVICE memory on the renderer's device; (W, H) must be the
 * camera's resolution.  `weights_in_or_null`: dense float32 (W,H) in DEVICE memory; `weights_out`: DEVICE memory, W * H floats (it may
 * be `weights_in_or_null`).  `counts_or_null`: HOST uint64 [4]; asking for counts makes the call wait for them, without them the call
 * returns when the kernel is queued behind everything the library has queued so far. */
int smesh_view_weights(smesh_renderer_t* renderer, const smesh_camera_t* camera, const uint32_t* indices_dev, const float* depth_dev,
                       uint64_t W, uint64_t H, const smesh_view_weights_spec_t* spec, const float* weights_in_or_null,
                       float* weights_out, uint64_t* counts_or_null);

/* smesh_fuse_views (smesh_fuse_views_probs16 / smesh_fuse_views_labels for the other image kinds) with every view weighted by its
 * viewing geometry, and -- where `gate_or_null` is given -- gated by its sensor depth as well.  `images`, `image_kind`,
 * `weights_or_null`: as smesh_fuse_views_depth.  `sensors_or_null` .. `gate_or_null`: the sensor arguments of smesh_fuse_views_depth,
 * all of them or none (sensors_or_null and gate_or_null both NULL; the others are then ignored).  `view_counts_or_null`: HOST uint64
 * [n][4] of this header; `depth_counts_or_null`: HOST uint64 [n][4] of smesh_depth.h, only with a gate; asking for either makes the
 * call wait.
 * Per group of up to eight views: the views are rasterised with their depth planes, ONE k_view_weights launch writes their weights
 * planes (library-owned) from `weights_or_null`, with a gate ONE k_depth_weights launch then gates those planes in place, and the
 * group's ordinary fusion launches read them as their weights -- under the conditions and with the kernels of smesh_fuse_views_depth.
 * The order view weights -> depth gate is part of the rule; a zero stays zero, so the depth counts are those of the gate alone. */
int smesh_fuse_views_view_weights(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                  const void* const* images, int image_kind, const float* const* weights_or_null,
                                  const smesh_view_weights_spec_t* spec,
                                  const void* const* sensors_or_null, int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind,
                                  uint64_t w, uint64_t h, const smesh_depth_gate_t* gate_or_null,
                                  uint64_t* view_counts_or_null, uint64_t* depth_counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_VIEW_WEIGHTS_H */
