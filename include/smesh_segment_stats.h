/*
 * smesh_segment_stats.h -- fused votes and areas pooled over the segments of a labelled mesh, of libsmesh_hip.so: an extension of the
 * C ABI in smesh.h on top of the segments of smesh_face_segments.h.
 *
 * smesh_face_segments.h says which faces belong together.  The entry points below add up what those faces carry, on the device:
 * every segment's pooled rows (its evidence, its argmax, its total), the same broadcast back to the segment's faces (region
 * voting: one label per crease-bounded patch), every face's and every segment's area, and a despeckle by any per-segment measure
 * (an area in square metres instead of a face count).  The reference has no such step.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * THE RULE, to the bit.  All arithmetic is single float32 operations, never fused.  There are no float atomics anywhere.  No result
 * depends on scheduling.  Two calls agree in every bit.
 *   members     members(s) is the faces f with ids[f] == s, in ascending f.  n_s = size[s].  The RANK of a member is its position in
 *               that list.
 *   term        term(f,c) = rows[f,c] without face weights.  With weights w float32[F] it is w[f] * rows[f,c]: one multiplication.
 *   chunk sums  Chunk j of s is its members of rank 256 j .. 256 j + 255.  p(s,j,c) starts from +0.0f and adds the chunk's terms one
 *               after another, in ascending rank.
 *   pooled      pooled(s,c) starts from +0.0f and adds p(s,j,c) one after another, in ascending j.  For n_s <= 256 this is the
 *               plain ascending sum, which is smesh_vertices.h's rule for a vertex.
 *   finish      The [S,C] array `pooled` is treated exactly as vertex rows are in smesh_vertices.h: SMESH_VTX_SUMS /
 *               SMESH_VTX_ANNOTATIONS, dont_care_threshold, out_rows and/or out_labels.
 *   face form   X[f,:] = pooled[ids[f],:] where ids[f] >= 0.  Otherwise X[f,:] = rows[f,:], unweighted and bit for bit.  X is then
 *               finished the same way, over F rows.
 *   face areas  n and l are exactly those of "THE NORMAL WEIGHTS" in smesh_face_graph.h: e1, e2, the cross product from two products
 *               and one difference per component, and l = sqrtf((nx*nx + ny*ny) + nz*nz).  area[f] = 0.5f * l.  A face without area
 *               gives +0.0f.  A non-finite vertex gives whatever IEEE gives.
 *   segment areas  `pooled` with C = 1, rows = area[:,None] and no weights.
 *   despeckle by a measure  The inputs are measure float32[S] and minimum float32.  A face is KEPT when it is labelled and
 *               measure[ids[f]] >= minimum.  This is false for a NaN on either side.  The labels form and the rows form are those of
 *               smesh_face_segments.h.  Removed faces are the labelled faces that are not kept.  Removed segments are the segments
 *               whose measure fails.
 *   member table  offsets is uint32[S+1], the exclusive scan of size.  members is uint32[labelled], the lists back to back.  All
 *               integers.
 * Rows are expected to be free of NaN.  A NaN does not hang or fault anything.
 *
 * The member table is built on the first call that needs it (a stable sort of the labelled faces by segment) and kept in the
 * segments handle, which is why those calls take the handle without `const`.
 *
 * Conventions are those of smesh.h and smesh_face_segments.h: every function returns a status, SMESH_ERR_INVALID for a bad argument
 * (NULL, a bad memory kind, a bad mode, no output, P != F, different devices, C == 0, a reduce-scattered accumulator).  Every call
 * returns when its outputs are complete.  No call writes to its inputs.
 */
#ifndef SMESH_SEGMENT_STATS_H
#define SMESH_SEGMENT_STATS_H

#include "smesh.h"
#include "smesh_face_graph.h"
#include "smesh_face_segments.h"
#include "smesh_vertices.h"

#ifdef __cplusplus
extern "C" {
#endif

/* area[f] of every face.  `faces`: HOST int32[F,3], the array `graph` was built from (an index outside [0, V): SMESH_ERR_INVALID);
 * `vertices`: float32[V,3] in `vertices_memkind`; `out_areas`: float32[F] in `out_memkind`. */
int smesh_segment_stats_face_areas(const smesh_face_graph_t* graph, const int32_t* faces, const float* vertices, int vertices_memkind,
                                   float* out_areas, int out_memkind);

/* Copies of the member table in `out_memkind`: offsets uint32[S+1], members uint32[labelled]; each may be NULL. */
int smesh_segment_stats_members(smesh_face_segments_t* segments, uint32_t* offsets, uint32_t* members, int out_memkind);

/* `pooled`, finished.  `rows`: float32[F,C] in `rows_memkind`; `face_weights`: float32[F] in `weights_memkind`, or NULL; `mode`:
 * SMESH_VTX_SUMS or SMESH_VTX_ANNOTATIONS; `out_rows`: float32[S,C] or NULL, `out_labels`: int32[S] or NULL, both in `out_memkind`,
 * at least one of them. */
int smesh_segment_stats_pool(smesh_face_segments_t* segments, const float* rows, int rows_memkind, uint32_t C, const float* face_weights,
                             int weights_memkind, int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels,
                             int out_memkind);

/* The face form: `out_rows`: float32[F,C] or NULL, `out_labels`: int32[F] or NULL. */
int smesh_segment_stats_pool_faces(smesh_face_segments_t* segments, const float* rows, int rows_memkind, uint32_t C,
                                   const float* face_weights, int weights_memkind, int mode, float dont_care_threshold, float* out_rows,
                                   int32_t* out_labels, int out_memkind);

/* Both on what smesh_aggregator_get would return, which stays on the device, with the aggregator's C.  The aggregator's primitives
 * must be the segments' faces (P == F) and both must live on one device.  Like get(): a pending row exchange is joined first, and a
 * reduce-scattered accumulator is refused. */
int smesh_aggregator_segment_stats_pool(smesh_aggregator_t* aggregator, smesh_face_segments_t* segments, const float* face_weights,
                                        int weights_memkind, int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels,
                                        int out_memkind);
int smesh_aggregator_segment_stats_pool_faces(smesh_aggregator_t* aggregator, smesh_face_segments_t* segments, const float* face_weights,
                                              int weights_memkind, int mode, float dont_care_threshold, float* out_rows,
                                              int32_t* out_labels, int out_memkind);

/* The despeckle by a measure, labels form.  `measure`: float32[S] in `measure_memkind`; `out_labels`: int32[F] in `out_memkind`;
 * `removed_faces`, `removed_segments`: one HOST uint64 each, or NULL. */
int smesh_segment_stats_despeckle_labels(const smesh_face_segments_t* segments, const float* measure, int measure_memkind, float minimum,
                                         int32_t* out_labels, int out_memkind, uint64_t* removed_faces, uint64_t* removed_segments);

/* The rows form: `rows` float32[F,C] in `rows_memkind`, `out_rows` float32[F,C] in `out_memkind`. */
int smesh_segment_stats_despeckle_rows(const smesh_face_segments_t* segments, const float* measure, int measure_memkind, float minimum,
                                       const float* rows, int rows_memkind, uint32_t C, float* out_rows, int out_memkind);

/* The rows form on what smesh_aggregator_get would return; P == F, one device, get()'s rules, as above. */
int smesh_aggregator_segment_stats_despeckle(smesh_aggregator_t* aggregator, const smesh_face_segments_t* segments, const float* measure,
                                             int measure_memkind, float minimum, float* out_rows, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_SEGMENT_STATS_H */
