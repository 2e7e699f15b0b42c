/*
 * smesh_points.h -- fused results for points that are not the mesh's vertices: an extension of the C ABI in smesh.h.
 *
 * The reference's evaluation has per-vertex metrics only when the fused mesh IS the ground-truth mesh
 * (eval-scannet/eval_scannet.py:245).  What is missing for a simplified mesh, a COLMAP mesh or a texel renderer's re-ordered
 * faces is a map from arbitrary points -- the ground truth's vertices, a lidar scan -- to the faces that were fused.  The entry
 * points below give it: a surface index (a uniform grid over the faces, built on the device), the closest face of every query
 * point, and the gather of the fused rows of those faces, straight from an aggregator if wanted.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * The closest face is defined to the bit.  Everything is IEEE float32, every operation rounded on its own (no fused
 * multiply-add), division correctly rounded.  For a query point q and a face f with the vertices a, b, c:
 *
 *   dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z
 *   ab=b-a  ac=c-a  ap=q-a  bp=q-b  cp=q-c
 *   d1=dot(ab,ap) d2=dot(ac,ap) d3=dot(ab,bp) d4=dot(ac,bp) d5=dot(ab,cp) d6=dot(ac,cp)
 *   vc=d1*d4-d3*d2   vb=d5*d2-d1*d6   va=d3*d6-d5*d4
 *   the first condition that holds gives the closest point r:
 *    1  d1<=0 && d2<=0                       r = a
 *    2  d3>=0 && d4<=d3                      r = b
 *    3  vc<=0 && d1>=0 && d3<=0              r = a + (d1/(d1-d3))*ab
 *    4  d6>=0 && d5<=d6                      r = c
 *    5  vb<=0 && d2>=0 && d6<=0              r = a + (d2/(d2-d6))*ac
 *    6  va<=0 && (d4-d3)>=0 && (d5-d6)>=0    r = b + ((d4-d3)/((d4-d3)+(d5-d6)))*(c-b)
 *    7  otherwise   den = 1/((va+vb)+vc);    r = (a + ab*(vb*den)) + ac*(vc*den)
 *   e = q-r;  dist2(q,f) = dot(e,e)
 *
 * The closest face of q is the face with the smallest dist2(q,f), the lowest f among equal values: starting from (+inf, -1), a
 * candidate replaces the best when dist2 < best, or dist2 == best && f < best_f.  A NaN or +inf distance never wins (degenerate
 * faces in case 7, faces with a NaN vertex; a face with an INFINITE vertex can still answer from a finite one through cases 1, 2
 * and 4, exactly as the rule says).  With max_distance = R >= 0, a point whose best dist2 does not satisfy
 * dist2 <= R*R (the float32 product; R = +inf: no limit) gets face -1 and dist2 +inf.  So does a point with a non-finite
 * coordinate, and every point when the mesh has no faces.
 *
 * The result is that of the exhaustive scan over all F faces; the index only makes it faster.
 *
 * Conventions are those of smesh.h: arrays are dense and row-major, every function returns a status, SMESH_ERR_INVALID for a bad
 * argument.  Every call returns when its outputs are complete.  Limits: 3 F and N below 2^32.
 */
#ifndef SMESH_POINTS_H
#define SMESH_POINTS_H

#include "smesh_vertices.h"   /* SMESH_VTX_SUMS, SMESH_VTX_ANNOTATIONS */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smesh_surface_index smesh_surface_index_t;

/* The index of the mesh `vertices` (HOST float32[V,3]), `faces` (HOST int32[F,3]), built on `device`: a uniform grid over the
 * bounding box of the finite vertices, about one cell per face, each dimension in [1, 256].  A face index outside [0, V):
 * SMESH_ERR_INVALID.  Faces with a non-finite vertex, faces without area and faces whose box overlaps too many cells are in no
 * cell: every query tests them. */
int smesh_surface_index_create(const float* vertices, uint64_t V, const int32_t* faces, uint64_t F, int device,
                               smesh_surface_index_t** out);
int smesh_surface_index_destroy(smesh_surface_index_t* index);
/* Faces, grid dimensions, entries of the cells' face lists, faces in the list that every query tests; every out pointer may be NULL. */
int smesh_surface_index_stats(const smesh_surface_index_t* index, uint64_t* F, uint32_t dims[3], uint64_t* entries,
                              uint64_t* large_faces);
/* The closest face of every point.  `points`: float32[N,3] in `points_memkind`; `max_distance`: R >= 0, +inf for no limit (a
 * negative or NaN value: SMESH_ERR_INVALID); `out_face`: int32[N], `out_dist2`: float32[N] or NULL, both in `out_memkind`.
 * The option "points_grid" (smesh_set_option; default 1) at 0 runs the exhaustive scan instead of the grid walk: same results. */
int smesh_surface_index_nearest(const smesh_surface_index_t* index, const float* points, uint64_t N, int points_memkind,
                                float max_distance, int32_t* out_face, float* out_dist2, int out_memkind);

/* The rows of the closest faces.  `face_rows`: float32[F,C] in `rows_memkind`; `faces`: int32[N] in `faces_memkind`, every value
 * below F (a face >= F: SMESH_ERR_INVALID; a negative one: no face).  Point i is treated as a vertex row of smesh_vertices.h is:
 *   mode SMESH_VTX_SUMS        out_rows[i,:] = face_rows[faces[i],:], all zero without a face
 *   mode SMESH_VTX_ANNOTATIONS t = the sum of that row in float32, in ascending c, starting from 0; the point is "don't care"
 *                              when it has no face or t < dont_care_threshold, and then its row is all zero; otherwise
 *                              out_rows[i,:] = row / t
 *   out_labels[i]              the lowest c with the largest value of the row; -1 where the point is don't care.  Valid in either
 *                              mode, and it always applies the threshold.
 * `out_rows`: float32[N,C] or NULL, `out_labels`: int32[N] or NULL, both in `out_memkind`; at least one of them.  A call without
 * `out_rows` writes no [N,C] array anywhere. */
int smesh_point_gather(const float* face_rows, int rows_memkind, uint64_t F, uint32_t C, const int32_t* faces, uint64_t N,
                       int faces_memkind, int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind);

/* smesh_point_gather on what smesh_aggregator_get would return, which stays on the device (Sum, Summax and Mul alike); F is the
 * aggregator's primitive count, and device arrays must live on the aggregator's device.  Like get(): a pending row exchange is
 * joined first, and a reduce-scattered accumulator is refused. */
int smesh_aggregator_point_annotations(smesh_aggregator_t* aggregator, const int32_t* faces, uint64_t N, int faces_memkind, int mode,
                                       float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_POINTS_H */
