/*
 * smesh_face_segments.h -- the connected components of a labelled mesh, of libsmesh_hip.so: an extension of the C ABI in smesh.h
 * on top of the face graph of smesh_face_graph.h.
 *
 * A fused mesh is a set of regions: this wall, that chair, a speckle of three "table" faces in the middle of the floor.  The entry
 * points below say which faces belong together -- the connected components of equal labels over the face graph, numbered and
 * measured on the device -- and remove the components that are too small, so that smesh_face_graph_propagate in SMESH_FG_FILL mode
 * can let their surroundings grow back in.  The reference has no such step.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * THE RULE, to the bit.  Everything is an integer; no result depends on scheduling, and two calls agree in every bit.
 *   inputs      a face graph (F faces, nnz list entries), labels int32[F], optionally weights float32[nnz] in the CSR's order and a
 *               float min_weight.
 *   labelled    face f is labelled when labels[f] >= 0.  Any non-negative value counts; -1 and every other negative value is
 *               "don't care".
 *   links       entry k of face f, naming g, LINKS f and g when both are labelled, labels[f] == labels[g], and weights is NULL or
 *               weights[k] >= min_weight (a NaN weight, or a NaN min_weight, does not link).  Links are undirected: one linking
 *               entry in either face's list suffices, so asymmetric weights still link.  The weights of
 *               smesh_face_graph_normal_weights are symmetric in bits, so creases cut segments when they are passed.
 *   segment     a connected component of labelled faces under links.  first_face of a segment is its lowest face index; segments
 *               are numbered 0 .. S-1 in ascending first_face.
 *   results     ids[f] (int32): the number of f's segment, -1 for an unlabelled face.  Per segment: first_face uint32[S],
 *               label int32[S] (the label of its faces), size uint32[S] (its number of faces).
 *   despeckle   with min_faces: face f is KEPT when it is labelled and size[ids[f]] >= min_faces.
 *               labels form   out[f] = labels[f] if f is kept, else -1.
 *               rows form     for float32 [F, C] rows: out[f, :] = rows[f, :] unless f is labelled and not kept; then +0.0f in every
 *                             class.  The rows of unlabelled faces pass through untouched, bit for bit.
 *               removed faces = the labelled faces that are not kept; removed segments = the segments with size < min_faces.
 *   from rows   where the input is rows (an aggregator), labels is what the finishing step of smesh_vertices.h gives for every row
 *               with SMESH_VTX_ANNOTATIONS and dont_care_threshold: the class with the largest value, the lowest one among equals,
 *               -1 where the row's total is below the threshold.
 * Per-segment areas and per-segment vote sums need an ordered float reduction per segment; they are not part of this header but of
 * smesh_segment_stats.h, which states that reduction to the bit.
 *
 * Conventions are those of smesh.h and smesh_face_graph.h: every function returns a status, SMESH_ERR_INVALID for a bad argument
 * (NULL, a bad memory kind, P != F, different devices, C == 0, a reduce-scattered accumulator).  Every call returns when its
 * outputs are complete.  No call writes to its inputs.  F must stay below 2^31 because ids are int32.
 */
#ifndef SMESH_FACE_SEGMENTS_H
#define SMESH_FACE_SEGMENTS_H

#include "smesh.h"
#include "smesh_face_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Owns, on the graph's device: ids[F], a copy of labels[F], first_face[S], label[S], size[S].  It does not refer to the graph or
 * to any input after the call that made it. */
typedef struct smesh_face_segments smesh_face_segments_t;

/* The segments of `labels` (int32[F] in `labels_memkind`) over `graph`.  `weights`: float32[nnz] in `weights_memkind`, or NULL
 * (then `min_weight` is ignored). */
int smesh_face_segments_create(const smesh_face_graph_t* graph, const int32_t* labels, int labels_memkind, const float* weights,
                               int weights_memkind, float min_weight, smesh_face_segments_t** out);

/* smesh_face_segments_create on the labels of what smesh_aggregator_get would return ("from rows" above); the rows stay on the
 * device.  The aggregator's primitives must be the graph's faces (P == F) and both must live on one device.  Like get(): a pending
 * row exchange is joined first, and a reduce-scattered accumulator is refused. */
int smesh_aggregator_face_segments(smesh_aggregator_t* aggregator, const smesh_face_graph_t* graph, float dont_care_threshold,
                                   const float* weights, int weights_memkind, float min_weight, smesh_face_segments_t** out);

int smesh_face_segments_destroy(smesh_face_segments_t* segments);

/* Faces, segments and labelled faces; every out pointer may be NULL. */
int smesh_face_segments_size(const smesh_face_segments_t* segments, uint64_t* F, uint64_t* S, uint64_t* labelled);

/* Copies of the results in `out_memkind`: ids int32[F], first_face uint32[S], label int32[S], size uint32[S]; each may be NULL. */
int smesh_face_segments_get(const smesh_face_segments_t* segments, int32_t* ids, uint32_t* first_face, int32_t* label, uint32_t* size,
                            int out_memkind);

/* The labels form of the despeckle: `out_labels` int32[F] in `out_memkind`; `removed_faces`, `removed_segments`: one HOST uint64
 * each, or NULL. */
int smesh_face_segments_despeckle_labels(const smesh_face_segments_t* segments, uint32_t min_faces, int32_t* out_labels, int out_memkind,
                                         uint64_t* removed_faces, uint64_t* removed_segments);

/* The rows form: `rows` float32[F,C] in `rows_memkind`, `out_rows` float32[F,C] in `out_memkind`. */
int smesh_face_segments_despeckle_rows(const smesh_face_segments_t* segments, uint32_t min_faces, const float* rows, int rows_memkind,
                                       uint32_t C, float* out_rows, int out_memkind);

/* The rows form on what smesh_aggregator_get would return, which stays on the device; `out_rows`: float32[F,C] with the
 * aggregator's C.  P == F, one device, get()'s rules, as above. */
int smesh_aggregator_face_segments_despeckle(smesh_aggregator_t* aggregator, const smesh_face_segments_t* segments, uint32_t min_faces,
                                             float* out_rows, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_FACE_SEGMENTS_H */
