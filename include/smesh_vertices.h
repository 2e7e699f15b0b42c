/*
 * smesh_vertices.h -- per-vertex results of libsmesh_hip.so: an extension of the C ABI in smesh.h.
 *
 * The reference's evaluation reports per VERTEX (eval-scannet/eval_scannet.py:249-287): it builds a vertex-to-faces table in a
 * Python loop over every face, gathers the face distributions of each vertex's faces, sums them, marks "don't care" where the
 * sum is below 0.9 and renormalises.  The entry points below do that on the device: a vertex map (a vertex-to-faces CSR built
 * once per mesh), a gather over it, the same gather straight from an aggregator (nothing but the outputs crosses PCIe), and
 * the step that comes before it for texel renderers: texel rows summed to face rows.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * The sums are defined to the bit.  For vertex v, s[v,c] is the sum of face_rows[f,c] over the faces f of v in ASCENDING f,
 * accumulated in float32, one addition after another, starting from 0.  A face that names v twice counts once.
 *   mode SMESH_VTX_SUMS         out_rows = s
 *   mode SMESH_VTX_ANNOTATIONS  t = sum over c of s[v,c], in float32, in ascending c, starting from 0;
 *                               v is "don't care" when t < dont_care_threshold (the reference: 0.9), and then its row is all
 *                               zero; otherwise out_rows[v,:] = s[v,:] / t.  A vertex without faces is don't care, whatever the threshold.
 *   out_labels[v]               the lowest c with the largest s[v,c]; -1 where v is don't care.  Valid in either mode, and it
 *                               always applies the threshold.
 * Face rows are expected to be free of NaN.
 *
 * Conventions are those of smesh.h: row arrays are dense and row-major, every function returns a status, SMESH_ERR_INVALID
 * for a bad argument.  Every call returns when its outputs are complete.
 */
#ifndef SMESH_VERTICES_H
#define SMESH_VERTICES_H

#include "smesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMESH_VTX_SUMS        0
#define SMESH_VTX_ANNOTATIONS 1

typedef struct smesh_vertex_map smesh_vertex_map_t;

/* Vertex-to-faces CSR of `faces` (HOST int32[F,3]) over V vertices, built on `device`: the faces of each vertex are counted,
 * the counts scanned, the lists filled, and every list sorted by ascending face index.  A face index outside [0, V):
 * SMESH_ERR_INVALID.  3 F and V must stay below 2^32. */
int smesh_vertex_map_create(const int32_t* faces, uint64_t F, uint64_t V, int device, smesh_vertex_map_t** out);
int smesh_vertex_map_destroy(smesh_vertex_map_t* map);
/* Faces, vertices and list entries (3 F less the repeated vertices of degenerate faces); every out pointer may be NULL. */
int smesh_vertex_map_size(const smesh_vertex_map_t* map, uint64_t* F, uint64_t* V, uint64_t* nnz);
/* The CSR copied to the host: offsets[V + 1], faces[nnz]; the faces of vertex v are faces[offsets[v] .. offsets[v + 1]). */
int smesh_vertex_map_adjacency(const smesh_vertex_map_t* map, uint64_t* offsets, uint32_t* faces);

/* The gather defined at the top of this file.  `face_rows`: float32[F,C] in `rows_memkind`; `out_rows`: float32[V,C] or NULL,
 * `out_labels`: int32[V] or NULL, both in `out_memkind`; at least one of them.  A call without `out_rows` writes no [V,C]
 * buffer anywhere. */
int smesh_vertex_map_gather(const smesh_vertex_map_t* map, const float* face_rows, int rows_memkind, uint32_t C, int mode,
                            float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind);

/* smesh_vertex_map_gather on what smesh_aggregator_get would return, which stays on the device (Sum, Summax and Mul alike).
 * The aggregator's primitives must be the map's faces (P == F) and both must live on one device.  Like get(): a pending row
 * exchange is joined first, and a reduce-scattered accumulator is refused. */
int smesh_aggregator_vertex_annotations(smesh_aggregator_t* aggregator, const smesh_vertex_map_t* map, int mode,
                                        float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind);

/* Texel rows to face rows.  Face f of the renderer's layout (smesh_renderer_texel_layout) owns the texels
 * [first[f], first[f] + res[f] (res[f] + 1) / 2); its row is the float32 sum of those rows of `texel_rows` (float32[P,C], P the
 * renderer's primitives) in ascending texel order, one addition after another from 0, then treated by `mode` and
 * `dont_care_threshold` as a vertex row is.  `out_face_rows`: float32[F,C] in the layout's face order -- the order of the faces a
 * vertex map for this mesh is built from.  A renderer that is not a texel renderer: SMESH_ERR_INVALID. */
int smesh_renderer_texel_face_rows(smesh_renderer_t* texel_renderer, const float* texel_rows, int rows_memkind, uint32_t C,
                                   int mode, float dont_care_threshold, float* out_face_rows, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_VERTICES_H */
