// scan.inc.hpp -- the exclusive scan of uint32 counts that the count / scan / fill pipelines share (vertices.hip: the faces of every
// vertex; points.hip: the faces of every grid cell, the points of every grid cell).  Included inside the including file's anonymous
// namespace, after its `constexpr int kBlock = 256`.
#pragma once

static_assert(kBlock == 256, "the scan kernels are written for workgroups of 256");

// Exclusive scan of in[n] into out[n] in three launches: kScanTile elements per workgroup (four per thread), the workgroup totals by
// one workgroup, then the totals added back.
constexpr int kScanPer = 4;
constexpr int kScanTile = kBlock * kScanPer;

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t* lds, uint32_t* total) {
  const int t = threadIdx.x;
  lds[t] = x;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const uint32_t y = t >= d ? lds[t - d] : 0u;
    __syncthreads();
    lds[t] += y;
    __syncthreads();
  }
  const uint32_t incl = lds[t];
  *total = lds[kBlock - 1];
  __syncthreads();
  return incl - x;
}

__global__ __launch_bounds__(kBlock) void k_scan_tiles(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
                                                       uint32_t* __restrict__ tile_sums) {
  __shared__ uint32_t lds[kBlock];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
  uint32_t x[kScanPer], sum = 0;
  for (int i = 0; i < kScanPer; i++) {
    x[i] = base + i < n ? in[base + i] : 0u;
    sum += x[i];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan(sum, lds, &total);
  for (int i = 0; i < kScanPer; i++) {
    if (base + i < n) out[base + i] = run;
    run += x[i];
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_scan_sums(uint32_t* __restrict__ sums, uint64_t n) {   // one workgroup, in place
  __shared__ uint32_t lds[kBlock];
  uint32_t carry = 0;
  for (uint64_t base = 0; base < n; base += kBlock) {
    const uint64_t i = base + threadIdx.x;
    const uint32_t x = i < n ? sums[i] : 0u;
    uint32_t total;
    const uint32_t excl = block_exclusive_scan(x, lds, &total);
    if (i < n) sums[i] = carry + excl;
    carry += total;
  }
}

__global__ __launch_bounds__(kBlock) void k_scan_add(uint32_t* __restrict__ out, uint64_t n, const uint32_t* __restrict__ tile_sums) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] += tile_sums[i / kScanTile];
}

// out[0 .. n) = exclusive scan of in[0 .. n), queued on `st`; `tiles`: scratch of div_up(n, kScanTile) uint32.
inline void launch_exclusive_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* tiles, hipStream_t st) {
  const uint64_t ntiles = smesh::div_up(n, kScanTile);
  hipLaunchKernelGGL(k_scan_tiles, dim3((uint32_t)ntiles), dim3(kBlock), 0, st, in, out, n, tiles);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kBlock), 0, st, tiles, ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3((uint32_t)smesh::div_up(n, kBlock)), dim3(kBlock), 0, st, out, n, tiles);
}
