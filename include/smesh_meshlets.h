/*
 * smesh_meshlets.h -- the meshlet tables of the grouped rasteriser of libsmesh_hip.so: an extension of the C ABI in smesh.h.
 *
 * smesh_fuse_views rasterises up to eight views of one mesh per launch.  Where every triangle of the launch takes one lane (meshes
 * whose triangles measure a few pixels), a workgroup owns one block of SMESH_MESHLET_TRIS consecutive triangles of the renderer's
 * final face order, projects the distinct vertices of that block into LDS and sets its triangles up from there: there is no
 * per-view array of projected vertices and no vertex stage for such a launch.  The tables that say which vertices a block uses
 * depend on the mesh alone and are built once per renderer, on the host, by the function below (exposed so that it can be
 * tested without a device).
 *
 * Option "raster_meshlets" (smesh_set_option / smesh_get_option of smesh.h; 0 / 1, default from SMESH_RASTER_MESHLETS): 0 = every
 * grouped launch runs the vertex stage, kernel for kernel what the library did before it had meshlets; 1 = grouped launches of the
 * one-lane-per-triangle instances of a renderer that has tables read them.  Same fragments, same records, same results.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 */
#ifndef SMESH_MESHLETS_H
#define SMESH_MESHLETS_H

#include "smesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMESH_MESHLET_TRIS      256   /* triangles per block */
#define SMESH_MESHLET_MAX_VERTS 384   /* distinct vertices a block may use */

/* Tables of `faces` (int32[F][3], indices into V vertices), block b = triangles [256 b, min(F, 256 b + 256)):
 *   first[b] .. first[b + 1]  block b's distinct vertex ids in `ids`, ascending (`first`: ceil(F / 256) + 1 entries);
 *   tris[f]                   l0 | l1 << 10 | l2 << 20, the positions of triangle f's vertices in its block's list.
 * *has_meshlets = 0 (the tables are then not written) if a block uses more than SMESH_MESHLET_MAX_VERTS distinct vertices or a face
 * holds an index outside [0, V): such a mesh keeps the vertex stage, as a whole.  `ids_capacity`: entries `ids` has room for
 * (3 F always suffices); *ids_used: entries written.  SMESH_ERR_INVALID for NULL arguments or too small a capacity. */
int smesh_meshlets_build(const int32_t* faces, uint64_t F, uint64_t V, uint32_t* first, uint32_t* ids, uint64_t ids_capacity,
                         uint32_t* tris, uint64_t* ids_used, int* has_meshlets);

/* Which path the calling thread's last GROUPED raster launch (smesh_fuse_views and its relatives) took: "meshlets",
 * "vertex-stage", or "none" before the first one. */
const char* smesh_last_raster_path(void);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_MESHLETS_H */
