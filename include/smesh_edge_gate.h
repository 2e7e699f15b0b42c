/*
 * smesh_edge_gate.h -- fusion gated at OCCLUSION EDGES: weights computed on the device from the rendered depth plane alone, an
 * extension of smesh.h with the shape of smesh_depth.h.
 *
 * The best-known failure of projective label fusion is label bleeding across occlusion edges: a pose that is a few pixels off puts
 * the network's "chair" pixels on the wall faces just behind the chair's silhouette, and the wall's pixels on the chair's rim.  Those
 * pixels are not grazing (smesh_view_weights.h keeps them), and the depth gate of smesh_depth.h needs a sensor image that RGB-only
 * datasets do not have.  The standard cure needs only what the library holds after every render: a pixel is dropped when a depth
 * discontinuity lies within a few pixels of it.  The entry points below compute the weights image that does so -- the plane every
 * fusion kernel already multiplies into a pixel's contribution -- in one kernel (k_edge_weights, csrc/edge_weights.hip) between the
 * rasteriser and the fusion launch, for up to eight views per launch.
 *
 * THE RULE, to the bit.  A gate is six numbers: radius (integer, 1 .. SMESH_EDGE_MAX_RADIUS), abs_tol >= 0, rel_tol >= 0, and the
 * flags behind, front and silhouette, each 0 or 1.  For output pixel (X, Y) of a dense float32 (W, H) depth plane with y fastest, the
 * WINDOW is every pixel (X', Y') inside the image with |X' - X| <= radius and |Y' - Y| <= radius; the pixel itself is in it, pixels
 * outside the image do not exist.  A depth that is not finite (+inf from the rasteriser; NaN or -inf in a caller's plane) is
 * BACKGROUND.  Every arithmetic step is a single float32 IEEE operation, never fused:
 *   d    = depth[X, Y]
 *   lo   = min of the finite depths in the window
 *   hi   = max of the finite depths in the window
 *   bg   = some depth in the window is background
 *   t    = abs_tol + rel_tol * d          (a multiply, then an add)
 *   1. d is background                    -> weight 0, counted nowhere
 *   2. behind     and (d - lo) > t        -> behind,      weight 0   (a nearer surface close by: its labels bleed onto this pixel)
 *   3. front      and (hi - d) > t        -> front,       weight 0   (the rim of an occluder)
 *   4. silhouette and bg                  -> silhouette,  weight 0   (the rim against the sky)
 *   5. otherwise                             weight w_in  (the caller's weights plane at (X, Y), or 1.0f)
 * Counts per view: uint64 [visible, behind, front, silhouette]; visible = the pixels with finite d; a pixel is counted in at most one
 * of the other three, the first matching step wins.  With all three flags 0 the output is w_in in bits for every visible pixel.
 * Only compares, one subtraction, one multiply and one add decide, so the result is unique; tests/edge_gate_ref.py (numpy, brute
 * force over the window) decides.
 *
 * The kernel: a workgroup of 256 lanes takes a tile of SMESH_EDGE_TILE_X columns by SMESH_EDGE_TILE_Y rows plus a halo of `radius`
 * and loads its depth ONCE into LDS -- background as NaN, outside the image as +inf, which can win neither the minimum nor the
 * maximum nor set bg.  The windowed min, max and background flag are computed separably: along y into three LDS planes, then along x
 * -- 2 (2 radius + 1) steps per pixel instead of (2 radius + 1)^2.  Lanes run along y, the contiguous axis; in the x pass a lane owns
 * four consecutive rows, reads the planes in 16 bytes, and moves weights_in / weights_out in 16 bytes where those planes are 16-byte
 * aligned and H is a multiple of four, else one by one.  The view comes from the block index, so ONE launch serves a group of up to
 * eight views, each with its own (W, H).  Counts: ballot and population count per wave, one atomic add per wave and counter.  The
 * depth plane is never written, so weights_out may be weights_in.  LDS layout, registers and measurements: DESIGN.md 3.17.
 * Read-only: smesh_get_option("edge_weights_launches") counts the launches of the kernel in this process.
 *
 * PRODUCT-ONLY: the oracle implements nothing of this header.
 *
 * Refused with SMESH_ERR_INVALID and a message, before anything is changed: a radius outside 1 .. 8; a NaN or negative abs_tol or
 * rel_tol; a flag other than 0 or 1; W or H over 65536, or W * H >= 2^29; NULL planes; in smesh_fuse_views_weighted everything
 * smesh_depth.h and smesh_view_weights.h refuse about their own arguments, and a call with no stage at all.
 */
#ifndef SMESH_EDGE_GATE_H
#define SMESH_EDGE_GATE_H

#include "smesh.h"
#include "smesh_depth.h"
#include "smesh_view_weights.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMESH_EDGE_MAX_RADIUS 8
/* the tile of one workgroup of k_edge_weights, without its halo: columns (x) by rows (y) */
#define SMESH_EDGE_TILE_X 32
#define SMESH_EDGE_TILE_Y 64

typedef struct smesh_edge_gate {
  int32_t radius;      /* 1 .. SMESH_EDGE_MAX_RADIUS: the window is (2 radius + 1)^2 pixels */
  float   abs_tol;
  float   rel_tol;
  int32_t behind;      /* 0 / 1: drop a pixel with a nearer surface in its window */
  int32_t front;       /* 0 / 1: drop a pixel with a farther surface in its window */
  int32_t silhouette;  /* 0 / 1: drop a pixel with background in its window */
} smesh_edge_gate_t;

/* The weights plane of ONE view.  `depth`: dense float32 (W,H) in DEVICE memory on `device` (smesh_renderer_render_device's plane, or
 * any plane of the caller's); `weights_in_or_null`: dense float32 (W,H) in DEVICE memory; `weights_out`: DEVICE memory, W * H floats
 * (it may be `weights_in_or_null`).  `counts_or_null`: HOST uint64 [4]; asking for counts makes the call wait for them, without them
 * the call returns when the kernel is queued behind everything the library has queued so far.  No renderer is needed. */
int smesh_edge_weights(const float* depth, uint64_t W, uint64_t H, const smesh_edge_gate_t* gate, const float* weights_in_or_null,
                       float* weights_out, uint64_t* counts_or_null, int device);

/* smesh_fuse_views (smesh_fuse_views_probs16 / smesh_fuse_views_labels for the other image kinds) with every view's weights computed
 * by any non-empty subset of three stages: the viewing-geometry weights (`spec_or_null`, smesh_view_weights.h), the edge gate
 * (`edge_or_null`, this header) and the sensor-depth gate (`sensors_or_null` .. `gate_or_null`, all of them or none, smesh_depth.h).
 * The other arguments are those of smesh_fuse_views_view_weights.  `view_counts_or_null`, `edge_counts_or_null`,
 * `depth_counts_or_null`: HOST uint64 [n][4] of the stage's header, each only with its stage; asking for any makes the call wait.
 * Per group of up to eight views: the views are rasterised with their depth planes, then up to three launches run in the fixed order
 * view weights -> edge gate -> depth gate, the later ones in place on the planes (library-owned) the earlier one wrote, and the
 * group's ordinary fusion launches read those planes as their weights.  The order is part of the rule; a zero stays zero, so the
 * counts of each stage are those of that stage alone.  Without `spec_or_null` a texel renderer is accepted: the edge gate and the
 * depth gate need no face ids, and such a renderer's views are fused view by view from the same planes. */
int smesh_fuse_views_weighted(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                              const void* const* images, int image_kind, const float* const* weights_or_null,
                              const smesh_view_weights_spec_t* spec_or_null, const smesh_edge_gate_t* edge_or_null,
                              const void* const* sensors_or_null, int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind,
                              uint64_t w, uint64_t h, const smesh_depth_gate_t* gate_or_null,
                              uint64_t* view_counts_or_null, uint64_t* edge_counts_or_null, uint64_t* depth_counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_EDGE_GATE_H */
