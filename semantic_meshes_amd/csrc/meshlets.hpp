// meshlets.hpp -- per-block vertex tables of a renderer's triangles (meshlets.cpp; plain host C++, no device needed).
//
// The grouped small-triangle rasteriser (raster.hip: k_raster_frag_group_ml) gives every workgroup one block of kMeshletTris
// consecutive triangles -- in the renderer's FINAL face order -- and projects the block's vertices itself, into LDS, instead of
// gathering them from a per-view array that a vertex stage wrote first.  For that it needs, per block, the list of the distinct
// vertices its triangles use and, per triangle, where in that list its three vertices are.
#pragma once

#include <cstdint>
#include <vector>

namespace smesh {

constexpr uint32_t kMeshletTris = 256;       // triangles per block: the 256 lanes of a workgroup
constexpr uint32_t kMeshletMaxVerts = 384;   // distinct vertices a block may use: 9 KB of LDS as three doubles each (a grid block uses ~170)
constexpr uint32_t kMeshletIndexBits = 10;   // a local index in the packed word (kMeshletMaxVerts <= 1 << kMeshletIndexBits)

struct MeshletTables {
  std::vector<uint32_t> first;   // [blocks + 1] block b's vertex ids are ids[first[b] .. first[b + 1])
  std::vector<uint32_t> ids;     // global vertex ids, ascending inside a block
  std::vector<uint32_t> tris;    // [F] l0 | l1 << 10 | l2 << 20: positions of the triangle's vertices in its block's list
};

// False -- the renderer has no meshlets and keeps the vertex stage -- if a block uses more than kMeshletMaxVerts distinct vertices or
// any face holds an index outside [0, V) (the rasteriser drops such a face; a table has no entry for it).  One decision per mesh.
bool build_meshlets(const int32_t* faces, uint64_t F, uint64_t V, MeshletTables& out);

}  // namespace smesh
