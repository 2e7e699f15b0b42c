// Stand-alone driver of the meshlet builder (semantic_meshes_amd/csrc/meshlets.cpp): plain host C++ with its own main, meant to be
// compiled together with that file under -fsanitize=address,undefined and run on the CPU (tests/test_meshlets_host.py does so).
// It builds the tables of the shapes the Python test uses and checks them by decoding: exit status 0 and "meshlets driver ok".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../semantic_meshes_amd/csrc/meshlets.hpp"

using smesh::MeshletTables;

static std::vector<int32_t> grid_faces(int a, int b, uint64_t keep) {
  std::vector<int32_t> f;
  for (int i = 0; i < a; i++)
    for (int j = 0; j < b; j++) {
      const int32_t v00 = i * (b + 1) + j, v10 = v00 + (b + 1), v01 = v00 + 1, v11 = v10 + 1;
      const int32_t two[6] = {v00, v10, v01, v10, v11, v01};
      f.insert(f.end(), two, two + 6);
    }
  f.resize(3 * keep);
  return f;
}

static int check(const char* name, const std::vector<int32_t>& faces, uint64_t V, bool want) {
  const uint64_t F = faces.size() / 3;
  MeshletTables t;
  const bool has = smesh::build_meshlets(faces.data(), F, V, t);
  if (has != want) { std::printf("%s: has_meshlets = %d, expected %d\n", name, (int)has, (int)want); return 1; }
  if (!has) return 0;
  const uint64_t blocks = (F + smesh::kMeshletTris - 1) / smesh::kMeshletTris;
  if (t.first.size() != blocks + 1 || t.tris.size() != F || t.first[0] != 0 || t.first[blocks] != t.ids.size()) {
    std::printf("%s: table sizes\n", name);
    return 1;
  }
  for (uint64_t f = 0; f < F; f++) {
    const uint64_t b = f / smesh::kMeshletTris;
    const uint32_t count = t.first[b + 1] - t.first[b];
    if (count > smesh::kMeshletMaxVerts) { std::printf("%s: block %llu over the cap\n", name, (unsigned long long)b); return 1; }
    for (int k = 0; k < 3; k++) {
      const uint32_t local = (t.tris[f] >> (smesh::kMeshletIndexBits * k)) & ((1u << smesh::kMeshletIndexBits) - 1u);
      if (local >= count || (int32_t)t.ids[t.first[b] + local] != faces[3 * f + k]) {
        std::printf("%s: triangle %llu corner %d does not decode\n", name, (unsigned long long)f, k);
        return 1;
      }
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  bad += check("grid, F = 256 * 7 + 37", grid_faces(40, 23, 256 * 7 + 37), 41 * 24, true);
  bad += check("F < 256", grid_faces(6, 5, 60), 7 * 6, true);
  bad += check("F = 256", grid_faces(16, 8, 256), 17 * 9, true);
  bad += check("no faces", std::vector<int32_t>(), 10, true);
  {
    std::vector<int32_t> soup(3 * 700);                        // every triangle has three vertices of its own: 768 per block
    for (size_t k = 0; k < soup.size(); k++) soup[k] = (int32_t)k;
    bad += check("soup", soup, soup.size(), false);
  }
  {
    std::vector<int32_t> f = grid_faces(20, 10, 400);
    f[3 * 301 + 1] = 21 * 11;                                  // == V: one index out of range
    bad += check("index out of range", f, 21 * 11, false);
    f[3 * 301 + 1] = -1;
    bad += check("negative index", f, 21 * 11, false);
  }
  if (bad) return 1;
  std::printf("meshlets driver ok\n");
  return 0;
}
