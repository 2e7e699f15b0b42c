// nearest_rule.hpp -- the sampling rule of include/smesh_label_prep.h as the one device function that every kernel applying it calls
// (label_prep.hip, label_colors.hip, depth_weights.hip): nearest neighbour with half-pixel centres, in integers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace smesh {

// Per axis: i = ((2X + 1) n) div (2N).  n, N <= 65536: (2X + 1) n < 2^34 -- a 32-bit division where the product fits, which is every
// image below 32768 pixels a side, else a 64-bit one.
__device__ __forceinline__ uint32_t src_index(uint32_t X, uint32_t n, uint32_t N) {
  const uint64_t num = (uint64_t)(2u * X + 1u) * n;
  if ((num >> 32) == 0) return (uint32_t)num / (2u * N);
  return (uint32_t)(num / (2ull * N));
}

}  // namespace smesh
