// count.inc.hpp -- the counters that the kernels of face_segments.hip and segment_stats.hip share.  Included inside the including
// file's anonymous namespace, after its `constexpr int kWave = 64` and `constexpr int kBlock = 256`.
#pragma once

// Counters: a kernel that counts runs a capped grid (kCountBlocks workgroups striding over the items) and every workgroup adds its
// lanes' counts once.  One add per wave of a 1 M-face launch is 15 625 adds to one word, which took 0.19 ms whatever the kernel did
// besides (measured: k_seg_flatten, k_seg_despeckle_labels); 2 048 adds do not show.
constexpr uint32_t kCountBlocks = 2048;

__device__ __forceinline__ void block_count_add(uint32_t mine, unsigned long long* counter) {
  __shared__ uint32_t per_wave[kBlock / kWave];
  for (int d = kWave >> 1; d > 0; d >>= 1) mine += __shfl_xor(mine, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) per_wave[threadIdx.x / kWave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n = 0;
    for (int w = 0; w < kBlock / kWave; w++) n += per_wave[w];
    if (n) atomicAdd(counter, (unsigned long long)n);
  }
}

inline dim3 count_grid(uint64_t n) { return dim3((uint32_t)std::min<uint64_t>(smesh::div_up(n, kBlock), kCountBlocks)); }
