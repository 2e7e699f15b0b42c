// meshlets.cpp -- builds the per-block vertex tables of meshlets.hpp.  Plain host C++: no HIP header, no device.
#include "meshlets.hpp"

#include <algorithm>

#include "../../include/smesh_meshlets.h"

namespace smesh {

static_assert(kMeshletMaxVerts <= (1u << kMeshletIndexBits), "a local index must fit its field of the packed word");
static_assert(kMeshletTris == SMESH_MESHLET_TRIS && kMeshletMaxVerts == SMESH_MESHLET_MAX_VERTS, "the header documents these");

bool build_meshlets(const int32_t* faces, uint64_t F, uint64_t V, MeshletTables& out) {
  const uint64_t blocks = (F + kMeshletTris - 1) / kMeshletTris;
  out.first.assign(blocks + 1, 0u);
  out.ids.clear();
  out.tris.assign(F, 0u);
  uint32_t used[3 * kMeshletTris];
  for (uint64_t b = 0; b < blocks; b++) {
    const uint64_t f0 = b * kMeshletTris, f1 = std::min<uint64_t>(F, f0 + kMeshletTris);   // (the last block may be short)
    const uint32_t n = (uint32_t)(3 * (f1 - f0));
    for (uint32_t k = 0; k < n; k++) {
      const int32_t i = faces[3 * f0 + k];
      if (i < 0 || (uint64_t)i >= V) return false;
      used[k] = (uint32_t)i;
    }
    std::sort(used, used + n);
    const uint32_t count = (uint32_t)(std::unique(used, used + n) - used);
    if (count > kMeshletMaxVerts) return false;
    if (out.ids.size() + count > 0xFFFFFFFFull) return false;      // (offsets are 32-bit; F < 2^32 keeps this out of reach in practice)
    for (uint64_t f = f0; f < f1; f++) {
      uint32_t word = 0u;
      for (int k = 0; k < 3; k++) {
        const uint32_t local = (uint32_t)(std::lower_bound(used, used + count, (uint32_t)faces[3 * f + k]) - used);
        word |= local << (kMeshletIndexBits * k);
      }
      out.tris[f] = word;
    }
    out.ids.insert(out.ids.end(), used, used + count);
    out.first[b + 1] = (uint32_t)out.ids.size();
  }
  return true;
}

}  // namespace smesh

extern "C" int smesh_meshlets_build(const int32_t* faces, uint64_t F, uint64_t V, uint32_t* first, uint32_t* ids, uint64_t ids_capacity,
                                    uint32_t* tris, uint64_t* ids_used, int* has_meshlets) {
  if (!has_meshlets || !ids_used || (F && (!faces || !tris)) || !first || (ids_capacity && !ids)) return SMESH_ERR_INVALID;
  *has_meshlets = 0;
  *ids_used = 0;
  smesh::MeshletTables t;
  if (!smesh::build_meshlets(faces, F, V, t)) return SMESH_OK;
  if (t.ids.size() > ids_capacity) return SMESH_ERR_INVALID;
  std::copy(t.first.begin(), t.first.end(), first);
  std::copy(t.ids.begin(), t.ids.end(), ids);
  std::copy(t.tris.begin(), t.tris.end(), tris);
  *ids_used = t.ids.size();
  *has_meshlets = 1;
  return SMESH_OK;
}
