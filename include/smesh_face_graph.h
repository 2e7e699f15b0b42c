/*
 * smesh_face_graph.h -- mesh-graph operations of libsmesh_hip.so: an extension of the C ABI in smesh.h.
 *
 * Every other result of the library treats a face as independent of its neighbours.  The entry points below propagate fused rows
 * ALONG THE SURFACE, on the device: a face graph (for every face, the faces across its edges, a CSR built once per mesh), a
 * fixed number of averaging iterations over it that either smooth every face towards its neighbours or fill the faces that no view
 * observed from those that were, and per-entry weights from the agreement of the two faces' normals.  The reference has no such
 * step: its results end at colorize_mesh.py:83-84, where a face whose row sums to less than 0.9 is "don't care".
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * THE GRAPH, to the bit.  Face f = (v0, v1, v2) has the edge slots 0, 1, 2 = {v0,v1}, {v1,v2}, {v2,v0}, as unordered pairs.  A slot
 * whose two vertices are equal is skipped; so is a slot that names the same unordered pair as an earlier slot of the same face.
 * The list of f is, slot after slot, every face g != f that names both vertices of the slot (in any of its corners), in ASCENDING
 * g.  A face that shares two edges with f (a duplicate face) therefore appears twice, and a non-manifold edge contributes all its
 * other faces.  The graph is built from the vertex-to-faces CSR of smesh_vertices.h: for a slot {a,b} one thread walks the shorter
 * of the two vertices' ascending lists and keeps the faces that contain the other vertex (count per face, scan, fill).  Every face
 * writes only its own segment in the order the walk gives: no atomics, no sort, nothing depends on scheduling.  A hub vertex with
 * thousands of faces makes that one thread's walk long; this is accepted.
 *
 * THE PROPAGATION, to the bit.  All arithmetic is single float32 operations, never fused.  x_0 = face_rows; for t = 0 .. T-1:
 *   row total   tot_t[f] = the sum of x_t[f,c] in ascending c, from 0.0f.
 *   informed    entry k of face f, naming neighbour g, is informed at step t when tot_t[g] > 0.
 *   sums        over the INFORMED entries of f in list order, from 0.0f:
 *                 s[c] = s[c] + w[k] * x_t[g,c]   (one multiplication, then one addition)      d = d + w[k]
 *               without weights: s[c] = s[c] + x_t[g,c], and d is the number of informed entries converted to float.
 *               m[c] = s[c] / d when d > 0.
 *   SMESH_FG_SMOOTH (alpha in [0,1]; om = 1.0f - alpha, computed once on the host in float32)
 *               x_{t+1}[f,c] = om * x_0[f,c] + alpha * m[c]   (two products, one sum) when d > 0;  x_0[f,c] otherwise.
 *   SMESH_FG_FILL   a face with tot_0[f] >= observed_threshold keeps x_{t+1}[f,:] = x_0[f,:]; every other face takes m when d > 0
 *               and x_t[f,:] otherwise.  The observed region is fixed and the front advances one ring per iteration; because only
 *               informed neighbours enter the mean, a filled row has the magnitude of the rows it came from.
 * x_T is then treated exactly as a vertex row is in smesh_vertices.h: SMESH_VTX_SUMS / SMESH_VTX_ANNOTATIONS, dont_care_threshold,
 * out_rows and/or out_labels.  T = 0 is that finishing step on x_0.  "Unreached" counts the faces whose tot_T is not > 0.
 * Face rows are expected to be free of NaN and non-negative, weights finite and >= 0.
 *
 * THE NORMAL WEIGHTS, to the bit.  For face (v0, v1, v2): e1 = v1 - v0 and e2 = v2 - v0, per component;
 *   n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), each component two products and one difference;
 *   l = sqrtf((nx*nx + ny*ny) + nz*nz).  For entry (f, g):  q = ((nfx*ngx + nfy*ngy) + nfz*ngz) / (lf * lg);  with two_sided,
 *   q = fabsf(q);  q not > 0 (NaN from a face without area included) gives 0, q > 1 gives 1;  the weight is q multiplied by itself
 *   power - 1 times, left to right.  Division and square root are correctly rounded.
 *
 * Conventions are those of smesh.h: row arrays are dense and row-major, every function returns a status, SMESH_ERR_INVALID for a
 * bad argument.  Every call returns when its outputs are complete.  No call writes to its inputs.
 */
#ifndef SMESH_FACE_GRAPH_H
#define SMESH_FACE_GRAPH_H

#include "smesh.h"
#include "smesh_vertices.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMESH_FG_SMOOTH 0
#define SMESH_FG_FILL   1
#define SMESH_FG_MAX_POWER 16

typedef struct smesh_face_graph smesh_face_graph_t;

/* The face graph of `faces` (HOST int32[F,3]) over V vertices, built on `device`.  A face index outside [0, V):
 * SMESH_ERR_INVALID.  3 F, V and the number of entries must stay below 2^32. */
int smesh_face_graph_create(const int32_t* faces, uint64_t F, uint64_t V, int device, smesh_face_graph_t** out);
int smesh_face_graph_destroy(smesh_face_graph_t* graph);
/* Faces, vertices and list entries; every out pointer may be NULL. */
int smesh_face_graph_size(const smesh_face_graph_t* graph, uint64_t* F, uint64_t* V, uint64_t* nnz);
/* The CSR copied to the host: offsets[F + 1], neighbours[nnz]; the list of face f is neighbours[offsets[f] .. offsets[f + 1]). */
int smesh_face_graph_adjacency(const smesh_face_graph_t* graph, uint64_t* offsets, uint32_t* neighbours);

/* The propagation defined at the top of this file.  `face_rows`: float32[F,C] in `rows_memkind`; `weights`: float32[nnz] in the
 * CSR's order in `weights_memkind`, or NULL; `mode`: SMESH_FG_SMOOTH (`alpha`) or SMESH_FG_FILL (`observed_threshold`);
 * `out_mode`: SMESH_VTX_SUMS or SMESH_VTX_ANNOTATIONS; `out_rows`: float32[F,C] or NULL, `out_labels`: int32[F] or NULL, both in
 * `out_memkind`, at least one of them; `out_unreached`: one HOST uint64, or NULL.  The iterations run between buffers the library
 * owns for the length of the call. */
int smesh_face_graph_propagate(const smesh_face_graph_t* graph, const float* face_rows, int rows_memkind, uint32_t C,
                               const float* weights, int weights_memkind, int mode, uint32_t iterations, float alpha,
                               float observed_threshold, int out_mode, float dont_care_threshold, float* out_rows,
                               int32_t* out_labels, uint64_t* out_unreached, int out_memkind);

/* smesh_face_graph_propagate on what smesh_aggregator_get would return, which stays on the device (Sum, Summax and Mul alike).
 * The aggregator's primitives must be the graph's faces (P == F) and both must live on one device.  Like get(): a pending row
 * exchange is joined first, and a reduce-scattered accumulator is refused. */
int smesh_aggregator_face_propagate(smesh_aggregator_t* aggregator, const smesh_face_graph_t* graph, const float* weights,
                                    int weights_memkind, int mode, uint32_t iterations, float alpha, float observed_threshold,
                                    int out_mode, float dont_care_threshold, float* out_rows, int32_t* out_labels,
                                    uint64_t* out_unreached, int out_memkind);

/* One weight per CSR entry by the rule at the top of this file.  `faces`: HOST int32[F,3], the array the graph was built from (an
 * index outside [0, V): SMESH_ERR_INVALID); `vertices`: float32[V,3] in `vertices_memkind`; `power` in 1 .. SMESH_FG_MAX_POWER;
 * `out_weights`: float32[nnz] in `out_memkind`. */
int smesh_face_graph_normal_weights(const smesh_face_graph_t* graph, const int32_t* faces, const float* vertices,
                                    int vertices_memkind, uint32_t power, int two_sided, float* out_weights, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_FACE_GRAPH_H */
