// mesh_host.hpp -- the host plumbing that the mesh-side results share (vertices.hip, points.hip, face_graph.hip, face_segments.hip,
// segment_stats.hip): the device blocks of one call, inputs and outputs that live on the host or on the device, and the handles'
// destroy / adjacency / owner check.  Host code only.  Included by those five files and by nothing else.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/smesh_vertices.h"

namespace smesh {

// Device blocks of one call, given back when it returns.
struct TempBlocks {
  std::vector<void*> blocks;
  template <typename T>
  int alloc(T** out, size_t bytes) {
    void* p = nullptr;
    SMESH_HIP(dev_malloc(&p, std::max<size_t>(bytes, 16)));
    blocks.push_back(p);
    *out = static_cast<T*>(p);
    return SMESH_OK;
  }
  ~TempBlocks() { for (void* p : blocks) (void)dev_free(p); }
};

inline bool memkind_ok(int m) { return m == SMESH_MEM_HOST || m == SMESH_MEM_DEVICE; }

// `src` (`bytes` in `memkind`) on the device: itself, or a staged copy that lives as long as `tmp`.
template <typename T>
int on_device(DeviceCtx* ctx, TempBlocks& tmp, const T* src, size_t bytes, int memkind, const T** out) {
  *out = src;
  if (memkind == SMESH_MEM_DEVICE || bytes == 0) return SMESH_OK;
  T* staged = nullptr;
  SMESH_TRY(tmp.alloc(&staged, bytes));
  SMESH_HIP(hipMemcpyAsync(staged, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  *out = staged;
  return SMESH_OK;
}

// `bytes` of device memory queued into the caller's `dst` (in `memkind`); nothing for a null `dst`, zero bytes, or `dst` itself.
template <typename T>
int copy_out(T* dst, const T* d_src, size_t bytes, int memkind, hipStream_t st) {
  if (!dst || bytes == 0 || dst == d_src) return SMESH_OK;
  SMESH_HIP(hipMemcpyAsync(dst, d_src, bytes, memkind == SMESH_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  return SMESH_OK;
}

// A result in `out_memkind`.  `dev` is what the kernel writes: the caller's own pointer for device memory, a block of `tmp` for host
// memory, null where the caller's pointer is null.  copy_back() queues the copy to the host; the caller waits for the stream.
template <typename T>
struct Out {
  T* dev = nullptr;
  T* user = nullptr;
  size_t bytes = 0;
  int memkind = SMESH_MEM_DEVICE;
  int init(TempBlocks& tmp, T* user_, size_t bytes_, int memkind_) {
    dev = user = user_;
    bytes = bytes_;
    memkind = memkind_;
    if (user && memkind == SMESH_MEM_HOST) SMESH_TRY(tmp.alloc(&dev, bytes));
    return SMESH_OK;
  }
  int copy_back(hipStream_t st) const { return copy_out<T>(user, dev, bytes, memkind, st); }
};

// A handle's device made current; the caller's current device is what it was when this goes.
struct DeviceScope {
  int device, previous = -1;
  explicit DeviceScope(int device_) : device(device_) {
    (void)hipGetDevice(&previous);
    (void)hipSetDevice(device);
  }
  ~DeviceScope() {
    if (previous >= 0 && previous != device) (void)hipSetDevice(previous);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// A 32-bit CSR of the device on the host, its offsets widened: offsets[n_items + 1], list[nnz].
inline int csr_to_host(DeviceCtx* ctx, const uint32_t* d_offsets, uint64_t n_items, const uint32_t* d_list, uint64_t nnz, uint64_t* offsets,
                       uint32_t* list) {
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  std::vector<uint32_t> narrow(n_items + 1);
  SMESH_HIP(hipMemcpyAsync(narrow.data(), d_offsets, (n_items + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (nnz) SMESH_HIP(hipMemcpyAsync(list, d_list, nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
  SMESH_HIP(hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i <= n_items; i++) offsets[i] = narrow[i];
  return SMESH_OK;
}

// Inside a smesh_aggregator_with_final_rows callback: the aggregator lives where `owner` ("vertex map", "face graph", ...) lives and
// has one primitive per face of it.
inline int check_rows_owner(const char* prefix, const char* owner, const DeviceCtx* ctx, const DeviceCtx* owner_ctx, uint64_t P, uint64_t F) {
  if (ctx != owner_ctx) return fail(SMESH_ERR_INVALID, std::string(prefix) + ": aggregator and " + owner + " live on different devices");
  if (P != F)
    return fail(SMESH_ERR_INVALID, std::string(prefix) + ": the aggregator has " + std::to_string(P) + " primitives, the " + owner + " " +
                                       std::to_string(F) + " faces");
  return SMESH_OK;
}

// What every gather refuses first (`what`: "vertex gather" or "point gather").
inline int check_gather_args(const char* what, uint32_t C, int mode, const void* out_rows, const void* out_labels, int in_memkind,
                             int out_memkind) {
  const std::string w(what);
  if (C == 0) return fail(SMESH_ERR_INVALID, w + ": the class count must be positive");
  if (mode != SMESH_VTX_SUMS && mode != SMESH_VTX_ANNOTATIONS) return fail(SMESH_ERR_INVALID, w + ": mode must be SMESH_VTX_SUMS or SMESH_VTX_ANNOTATIONS");
  if (!out_rows && !out_labels) return fail(SMESH_ERR_INVALID, w + ": at least one of out_rows and out_labels is required");
  if (!memkind_ok(in_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, w + ": bad memory kind");
  return SMESH_OK;
}

}  // namespace smesh
