// fusion_multi8.hip -- the eight-views-per-launch instances of the triangle-order fusion kernel k_fuse_tri (class counts up to 40:
// exact instances 5 / 13 / 19 / 20 / 21 / 40, run-time-C instances sized 8 / 16 / 24 / 32 / 40).  A translation unit of its own so that the
// instance sets compile in parallel (see fusion_pair.hip).
#include <hip/hip_runtime.h>

#include "common.hpp"

#include <atomic>
#include <cmath>
#include <type_traits>

using namespace smesh;

namespace {

#include "fuse_tri.inc.hpp"

}  // namespace

// Static LDS and registers of the eight-view instance for (kind, tri_ct), from the code object: what the launch side needs to compute
// the pad that caps the launch beside the rasteriser (common.hpp: pipeline_fuse_pad).  False: the runtime would not say.
bool smesh_fuse_tri_8_resources(int kind, int tri_ct, uint32_t* static_lds, uint32_t* vgprs) {
  static std::atomic<uint64_t> known[3][64];     // static_lds << 32 | vgprs of (kind, slot); 0: not asked yet
  std::atomic<uint64_t>& slot = known[kind == SMESH_AGG_SUM ? 0 : kind == SMESH_AGG_SUMMAX ? 1 : 2][(unsigned)tri_ct & 63u];
  if (const uint64_t k = slot.load()) { *static_lds = (uint32_t)(k >> 32); *vgprs = (uint32_t)k; return true; }
  const void* fn = nullptr;
#define SMESH_FTR(K)                                                                   \
  switch (tri_ct) {                                                                     \
    case 5:  fn = reinterpret_cast<const void*>(&k_fuse_tri<5, K, true, 8>); break;     \
    case 13: fn = reinterpret_cast<const void*>(&k_fuse_tri<13, K, true, 8>); break;    \
    case 19: fn = reinterpret_cast<const void*>(&k_fuse_tri<19, K, true, 8>); break;    \
    case 20: fn = reinterpret_cast<const void*>(&k_fuse_tri<20, K, true, 8>); break;    \
    case 21: fn = reinterpret_cast<const void*>(&k_fuse_tri<21, K, true, 8>); break;    \
    case 40: fn = reinterpret_cast<const void*>(&k_fuse_tri<40, K, true, 8>); break;    \
    case 32: fn = reinterpret_cast<const void*>(&k_fuse_tri<32, K, false, 8>); break;   \
    case 41: fn = reinterpret_cast<const void*>(&k_fuse_tri<40, K, false, 8>); break;   \
    case 8:  fn = reinterpret_cast<const void*>(&k_fuse_tri<8, K, false, 8>); break;    \
    case 16: fn = reinterpret_cast<const void*>(&k_fuse_tri<16, K, false, 8>); break;   \
    default: fn = reinterpret_cast<const void*>(&k_fuse_tri<24, K, false, 8>); break;   \
  }
  switch (kind) {
    case SMESH_AGG_SUM: SMESH_FTR(SMESH_AGG_SUM); break;
    case SMESH_AGG_SUMMAX: SMESH_FTR(SMESH_AGG_SUMMAX); break;
    default: SMESH_FTR(SMESH_AGG_MUL); break;
  }
#undef SMESH_FTR
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return false; }
  *static_lds = (uint32_t)fa.sharedSizeBytes;
  *vgprs = (uint32_t)std::max(1, fa.numRegs);
  slot.store((uint64_t)*static_lds << 32 | *vgprs);
  return true;
}

void smesh_launch_fuse_tri_8(int kind, int tri_ct, dim3 grid, hipStream_t st, const TriFuseArgs& t, const TriViews<8>& tv) {
  const dim3 block(kWave);
  // Group pipeline (SMESH_GROUP_PIPELINE=0 / smesh_set_option turn it off; raster.hip): the rasteriser of the next group runs beside this launch, and the one-wave
  // workgroups of this kernel would take every wave slot that frees up.  An LDS pad caps them at five per CU -- alone the kernel
  // loses 2 % that way (it is bound by the memory system, not by occupancy) -- and leaves the rest of the register file to the
  // rasteriser's waves (NOTES/round2.md).
  const unsigned pad = t.lds_pad;      // (decided per launch: smesh_aggregator_fuse_triangles)
  TriViews<8> vn;
  for (int v = 0; v < 8; v++) vn.v[v] = tv.v[v];
#define SMESH_FTN(K)                                                                                     \
  switch (tri_ct) {                                                                                      \
    case 5:  hipLaunchKernelGGL((k_fuse_tri<5, K, true, 8>), grid, block, pad, st, t, vn); break;          \
    case 13: hipLaunchKernelGGL((k_fuse_tri<13, K, true, 8>), grid, block, pad, st, t, vn); break;         \
    case 19: hipLaunchKernelGGL((k_fuse_tri<19, K, true, 8>), grid, block, pad, st, t, vn); break;         \
    case 20: hipLaunchKernelGGL((k_fuse_tri<20, K, true, 8>), grid, block, pad, st, t, vn); break;         \
    case 21: hipLaunchKernelGGL((k_fuse_tri<21, K, true, 8>), grid, block, pad, st, t, vn); break;         \
    case 40: hipLaunchKernelGGL((k_fuse_tri<40, K, true, 8>), grid, block, pad, st, t, vn); break;         \
    case 32: hipLaunchKernelGGL((k_fuse_tri<32, K, false, 8>), grid, block, pad, st, t, vn); break;        \
    case 41: hipLaunchKernelGGL((k_fuse_tri<40, K, false, 8>), grid, block, pad, st, t, vn); break;        \
    case 8:  hipLaunchKernelGGL((k_fuse_tri<8, K, false, 8>), grid, block, pad, st, t, vn); break;         \
    case 16: hipLaunchKernelGGL((k_fuse_tri<16, K, false, 8>), grid, block, pad, st, t, vn); break;        \
    default: hipLaunchKernelGGL((k_fuse_tri<24, K, false, 8>), grid, block, pad, st, t, vn); break;        \
  }
  switch (kind) {
    case SMESH_AGG_SUM: SMESH_FTN(SMESH_AGG_SUM); break;
    case SMESH_AGG_SUMMAX: SMESH_FTN(SMESH_AGG_SUMMAX); break;
    default: SMESH_FTN(SMESH_AGG_MUL); break;
  }
#undef SMESH_FTN
}
