/*
 * smesh_label_images.h -- the fused mesh rendered back into the views as label and colour images, on the device: an extension of
 * the C ABI in smesh.h.
 *
 * The reference's workflow ends with "render the annotated mesh from original camera poses to produce new 2D consistent annotation
 * images" (README step 4; the `*_fused.png` images of eval-scannet/eval_scannet.py:318-320): render(), a gather of the (W,H,C)
 * float annotation image, an argmax, a palette lookup and a transpose on the host.  What the user wants per view is one byte per
 * pixel, or three for a colour image, in the orientation image encoders take.  One int32 label per primitive
 * (smesh_aggregator_labels, smesh_vertex_map_gather) and the rendered index plane give exactly that.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * Definitions (this project's; DESIGN.md "Label and colour images").  A label renderer holds a SNAPSHOT, taken at creation, of a
 * per-primitive int32 table labels[P], a class count K >= 1, an output label dtype -- SMESH_LBL_U8 (K <= 255) or SMESH_LBL_U16
 * (K <= 65535) --, a don't-care label `dc` (any value of that dtype), optionally a palette uint8 [K, 3] and a don't-care colour
 * uint8 [3].  For pixel (x, y) of an index image with value i, let l = labels[i] if 0 <= i < P and l = -1 otherwise (the background
 * 0xFFFFFFFF, negative values of the signed dtypes, indices >= P).  If 0 <= l < K the label output is l and the colour output is
 * palette[l]; otherwise they are `dc` and the don't-care colour.  Every output is an integer that depends on no launch shape.
 *
 * Output layouts:
 *   SMESH_LAYOUT_WH  the project's convention: element (x, y) at x * H + y, colours at (x * H + y) * 3 + channel
 *   SMESH_LAYOUT_HW  the image convention:     element (y, x) at y * W + x, colours at (y * W + x) * 3 + channel
 * Outputs are dense and may start at any byte address.
 *
 * Conventions are those of smesh_labels.h: index images are (W,H) with y fastest, strides in ELEMENTS, >= 0 and below 2^40 (NULL: dense), every
 * function returns a status, SMESH_ERR_INVALID comes with a message and with nothing written.  HOST outputs are complete when a
 * call returns (they are staged in device memory and copied at 1, 2 or 3 bytes per pixel); DEVICE outputs are asynchronous on the
 * library's main stream like the other entry points: valid after smesh_synchronize, smesh_stream_release or a completion token,
 * and a DEVICE index image must stay valid until then.
 */
#ifndef SMESH_LABEL_IMAGES_H
#define SMESH_LABEL_IMAGES_H

#include "smesh.h"
#include "smesh_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* smesh_profile_* slot of the image kernel (smesh.h leaves slots 6 and 7 free beside smesh_eval.h's 5). */
#define SMESH_PROF_LABEL_IMAGES 6

#define SMESH_LAYOUT_WH 0
#define SMESH_LAYOUT_HW 1

typedef struct smesh_label_renderer smesh_label_renderer_t;

/* Resolves the snapshot into a per-primitive device table on `device`.  `prim_labels`: int32 [P] in `labels_memkind` (read before
 * the call returns; may be NULL when P == 0, and then every pixel is don't care); P < 2^32 - 1.  `palette`: HOST uint8
 * [num_classes * 3] or NULL (no colour output); `dont_care_color`: HOST uint8 [3] or NULL (0, 0, 0). */
int smesh_label_renderer_create(const int32_t* prim_labels, uint64_t P, int labels_memkind,
                                uint32_t num_classes, int label_dtype, uint32_t dont_care_label,
                                const uint8_t* palette, const uint8_t dont_care_color[3],
                                int device, smesh_label_renderer_t** out);
int smesh_label_renderer_destroy(smesh_label_renderer_t* lr);

/* An index image that exists (smesh_renderer_render output, a cache) of `idx_dtype` (SMESH_IDX_*).  `labels_out`: W * H elements
 * of the label dtype, `colors_out`: W * H * 3 bytes, both in `out_memkind`; either may be NULL, not both; `colors_out` needs a
 * palette. */
int smesh_label_renderer_render_image(smesh_label_renderer_t* lr, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                      int idx_memkind, uint64_t W, uint64_t H, int layout,
                                      void* labels_out, uint8_t* colors_out, int out_memkind);

/* Rasterise `n` views and write one image per view; no index plane leaves HBM.  Groups of up to eight views share their rasteriser
 * launches, as in smesh_fuse_views, and -- where they share a resolution -- one launch of the image kernel.  `labels_out` /
 * `colors_out`: `n` pointers each, or NULL for the whole output (not both NULL unless n == 0).  The table's P must be the
 * renderer's primitive count (triangles or texels alike); that is checked before anything is written. */
int smesh_label_renderer_render_views(smesh_label_renderer_t* lr, smesh_renderer_t* renderer, const smesh_camera_t* cameras, uint64_t n,
                                      int layout, void* const* labels_out, uint8_t* const* colors_out, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_LABEL_IMAGES_H */
