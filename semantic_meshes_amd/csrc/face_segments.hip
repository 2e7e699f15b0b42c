// face_segments.hip -- the connected components of a labelled mesh (include/smesh_face_segments.h): a lock-free union-find over the
// face graph of face_graph.hip, the numbering of its roots, and the removal of segments that are too small.
//
// The reference has no such step.  Every other kernel of the mesh-graph files is a gather: one lane owns one output and reads its
// inputs.  Components need lanes to agree across a whole launch, so this file is written around four rules.
//
//   1. parent[x] <= x, always, and every write to parent strictly lowers a value.  The root of a finished component is therefore
//      its lowest face -- the header's first_face -- whatever the order of events, and every result is unique.
//   2. Inside the hooking launch every access to parent is an agent-scope relaxed atomic: the XCDs' L2s are not coherent with each
//      other and a CU's L1 is never refreshed by another CU's stores, so a plain load could be served from a stale line for ever.
//      Correctness does not rest on any load being fresh all the same: by rule 1 a stale parent is still an ancestor, and the
//      compare-and-swap on a ROOT (parent[hi] == hi -> lo) is the only thing that decides a union.
//   3. Nobody waits.  No grid barrier, no cooperative launch, no flag that a workgroup polls, no loop whose exit depends on another
//      lane's progress: every loop below ends because an unsigned value that the lane itself holds strictly decreased (stated at each).
//   4. The launch sequence is fixed: init, hook, flatten, flag + scan, number, count.  Nothing depends on the labels or on the mesh's
//      diameter; there is no "until nothing changed".
#include "mesh_host.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smesh_face_segments.h"
#include "../../include/smesh_vertices.h"

using namespace smesh;

struct smesh_face_segments {
  DeviceCtx* ctx = nullptr;
  uint64_t F = 0, S = 0, labelled = 0;
  int32_t* ids = nullptr;          // [F]
  int32_t* labels = nullptr;       // [F] a copy of the input
  uint32_t* first_face = nullptr;  // [S]
  int32_t* seg_label = nullptr;    // [S]
  uint32_t* size = nullptr;        // [S]
  SegmentMembers members;          // built on first use by segment_stats.hip, under the context lock
};

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;

#include "scan.inc.hpp"   // launch_exclusive_scan

// ---- the union-find ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Does entry k of face f (label lf >= 0), naming g, link the two?
__device__ __forceinline__ bool entry_links(const int32_t* __restrict__ labels, const float* __restrict__ w, float min_weight, int32_t lf,
                                            uint32_t g, uint32_t k) {
  if (labels[g] != lf) return false;
  return w == nullptr || w[k] >= min_weight;      // (false for a NaN on either side)
}

// parent[f] = the lowest face below f that an entry of f's own list links it to, or f.  Plain stores: the launch boundary publishes
// them.  A valid start: the edge is a link, so f and that face belong to one segment, and the value is < f.
__global__ __launch_bounds__(kBlock) void k_seg_init(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbr,
                                                     const int32_t* __restrict__ labels, const float* __restrict__ w, float min_weight,
                                                     uint64_t F, uint32_t* __restrict__ parent) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  uint32_t lowest = (uint32_t)f;
  const int32_t lf = labels[f];
  if (lf >= 0) {
    for (uint32_t k = offsets[f]; k < offsets[f + 1]; k++) {
      const uint32_t g = nbr[k];
      if (g < lowest && entry_links(labels, w, min_weight, lf, g, k)) lowest = g;
    }
  }
  parent[f] = lowest;
}

// The root above x, halving the path on the way (every second face is pointed at its grandparent).  The halving writes are
// atomicMin of an ancestor: they lower a value or do nothing, and they touch only faces that are no longer roots.
// TERMINATION: x takes the value of a parent that differs from it, and parent[x] <= x, so x strictly decreases with every turn; it
// is bounded by 0.  The loop reads what other lanes wrote but never waits for it: any value it can read ends or shortens the walk.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  uint32_t p = parent_load(parent + x);
  while (p != x) {
    const uint32_t gp = parent_load(parent + p);
    if (gp != p) (void)__hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = gp;
  }
  return x;
}

// Makes a and b, two faces that a link joins, members of one tree.
// TERMINATION: a turn either returns (equal roots, or the compare-and-swap made the higher root a child of the lower), or the
// compare-and-swap failed and returned the value `seen` that another lane stored in parent[hi]: seen < hi by rule 1.  The next
// turn starts from (seen, lo) -- from the returned value, never from a re-read -- and find_root only lowers what it is given, so
// the pair's higher member strictly decreases from turn to turn; it is bounded by 0.  A lane that fails has lost to a lane that
// succeeded, so the launch as a whole makes progress too, but no lane's exit depends on that.
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);      // agent scope, relaxed: only a root is ever re-pointed
    if (seen == hi) return;
    a = seen;                                                   // hi has a parent now; that parent and lo are to be joined
    b = lo;
  }
}

// One lane owns face f and walks its list.  Links are undirected and without weights both directions of an edge link alike, so the
// entry with g < f does the work of both.  With weights the reverse entry may fail where this one passes, and the reverse entry is
// somewhere in g's list: every linking entry is processed, whichever way it points (a union that is already made costs two walks).
__global__ __launch_bounds__(kBlock) void k_seg_hook(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbr,
                                                     const int32_t* __restrict__ labels, const float* __restrict__ w, float min_weight,
                                                     uint64_t F, uint32_t* parent) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int32_t lf = labels[f];
  if (lf < 0) return;
  const uint32_t end = offsets[f + 1];
  for (uint32_t k = offsets[f]; k < end; k++) {                 // (a list: k only counts up to `end`)
    const uint32_t g = nbr[k];
    if (w == nullptr && g > (uint32_t)f) continue;
    if (entry_links(labels, w, min_weight, lf, g, k)) unite(parent, (uint32_t)f, g);
  }
}

#include "count.inc.hpp"  // kCountBlocks, block_count_add, count_grid

// After the launch boundary plain loads are fresh.  root[f] = the root above f (a separate array: nobody reads what this launch
// writes); flag[f] = 1 for a labelled root -- a segment's first face -- and flag[F] = 0, so that the exclusive scan over F + 1
// elements ends in the number of segments.  The labelled faces are counted on the way.
// TERMINATION: as find_root, over values that no longer change; the outer loop strides over F + 1 items.
__global__ __launch_bounds__(kBlock) void k_seg_flatten(const uint32_t* __restrict__ parent, const int32_t* __restrict__ labels, uint64_t F,
                                                        uint32_t* __restrict__ root, uint32_t* __restrict__ flag,
                                                        unsigned long long* __restrict__ labelled) {
  uint32_t mine = 0;
  for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f <= F; f += (uint64_t)gridDim.x * kBlock) {
    if (f == F) {
      flag[f] = 0u;
      break;
    }
    uint32_t x = (uint32_t)f, p = parent[x];
    while (p != x) {
      x = p;
      p = parent[x];
    }
    root[f] = x;
    const bool lab = labels[f] >= 0;
    flag[f] = lab && x == (uint32_t)f ? 1u : 0u;
    mine += lab ? 1u : 0u;
  }
  block_count_add(mine, labelled);
}

// number[x] (the exclusive scan of flag) is the segment number of a first face x.
__global__ __launch_bounds__(kBlock) void k_seg_number(const uint32_t* __restrict__ root, const uint32_t* __restrict__ number,
                                                       const int32_t* __restrict__ labels, uint64_t F, int32_t* __restrict__ ids,
                                                       uint32_t* __restrict__ first_face, int32_t* __restrict__ seg_label,
                                                       uint32_t* __restrict__ size) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool counts = false;
  uint32_t s = 0;
  if (f < F) {
    const int32_t lf = labels[f];
    if (lf < 0) {
      ids[f] = -1;
    } else {
      const uint32_t r = root[f];
      s = number[r];
      counts = true;
      ids[f] = (int32_t)s;
      if (r == (uint32_t)f) {
        first_face[s] = r;
        seg_label[s] = lf;
      }
    }
  }
  // Sizes: integer adds, the same sum in any order.  Up to kSizeRounds times the lanes that share the segment of the wave's first
  // lane still to count add once, together; what is left adds one by one.  Under one giant segment a million adds would otherwise
  // land on one word: measured on the 1 M-triangle mesh, constant labels, 11.8 ms for the whole call with one add per face against
  // 0.67 ms with one round.  The loop is uniform across the wave and runs at most kSizeRounds times.
  constexpr int kSizeRounds = 4;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  unsigned long long todo = __ballot(counts);
  for (int round = 0; round < kSizeRounds && todo; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t ls = __shfl(s, leader, kWave);
    const unsigned long long same = __ballot(counts && s == ls);      // (a lane that has counted has another segment than the leader)
    if (lane == leader) atomicAdd(size + ls, (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(size + s, 1u);
}

// ---- the despeckle: plain gathers ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_despeckle_labels(const int32_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                                 const uint32_t* __restrict__ size, uint32_t min_faces, uint64_t F,
                                                                 int32_t* __restrict__ out, unsigned long long* __restrict__ removed) {
  uint32_t mine = 0;
  for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < F; f += (uint64_t)gridDim.x * kBlock) {
    const int32_t lf = labels[f];
    const bool kept = lf >= 0 && size[ids[f]] >= min_faces;
    mine += lf >= 0 && !kept ? 1u : 0u;
    out[f] = kept ? lf : -1;
  }
  block_count_add(mine, removed);
}

__global__ __launch_bounds__(kBlock) void k_seg_small(const uint32_t* __restrict__ size, uint32_t min_faces, uint64_t S,
                                                      unsigned long long* __restrict__ removed) {
  uint32_t mine = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kBlock) mine += size[s] < min_faces ? 1u : 0u;
  block_count_add(mine, removed);
}

__device__ __forceinline__ bool face_removed(const int32_t* __restrict__ ids, const uint32_t* __restrict__ size, uint32_t min_faces, uint64_t f) {
  const int32_t s = ids[f];
  return s >= 0 && size[s] < min_faces;
}

// T = float4: one lane per 16 bytes (C a multiple of four, both arrays aligned), `per_row` = C / 4; T = float: one lane per element.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_seg_despeckle_rows(const T* __restrict__ rows, const int32_t* __restrict__ ids,
                                                               const uint32_t* __restrict__ size, uint32_t min_faces, uint64_t n,
                                                               uint32_t per_row, T* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T v = rows[i];
  if (face_removed(ids, size, min_faces, i / per_row)) v = T{};      // +0.0f in every class
  out[i] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
dim3 grid_for(uint64_t n) { return dim3((uint32_t)div_up(n, kBlock)); }

void free_segments(smesh_face_segments* sg) {
  for (void* p : {(void*)sg->ids, (void*)sg->labels, (void*)sg->first_face, (void*)sg->seg_label, (void*)sg->size, (void*)sg->members.offsets,
                  (void*)sg->members.members, (void*)sg->members.chunk_start, (void*)sg->members.partial_start})
    if (p) (void)dev_free(p);
  delete sg;
}

// The segments of `sg->labels` (on the device already, F of them) over the graph's tables.  Context locked, device current.
int build_segments(smesh_face_segments* sg, const uint32_t* offsets, const uint32_t* nbr, const float* d_w, float min_weight) {
  DeviceCtx* ctx = sg->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t F = sg->F, n = F + 1;
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&sg->ids), std::max<uint64_t>(F * 4, 16)));
  if (F == 0) {
    SMESH_HIP(hipStreamSynchronize(st));
    return SMESH_OK;
  }
  TempBlocks tmp;
  uint32_t *parent = nullptr, *root = nullptr, *flag = nullptr, *number = nullptr, *tiles = nullptr;
  unsigned long long* labelled = nullptr;
  SMESH_TRY(tmp.alloc(&parent, F * 4));
  SMESH_TRY(tmp.alloc(&root, F * 4));
  SMESH_TRY(tmp.alloc(&flag, n * 4));
  SMESH_TRY(tmp.alloc(&number, n * 4));
  SMESH_TRY(tmp.alloc(&tiles, div_up(n, kScanTile) * 4));
  SMESH_TRY(tmp.alloc(&labelled, 16));
  SMESH_HIP(hipMemsetAsync(labelled, 0, 16, st));
  const dim3 gf = grid_for(F), b(kBlock);
  hipLaunchKernelGGL(k_seg_init, gf, b, 0, st, offsets, nbr, (const int32_t*)sg->labels, d_w, min_weight, F, parent);
  hipLaunchKernelGGL(k_seg_hook, gf, b, 0, st, offsets, nbr, (const int32_t*)sg->labels, d_w, min_weight, F, parent);
  hipLaunchKernelGGL(k_seg_flatten, count_grid(n), b, 0, st, (const uint32_t*)parent, (const int32_t*)sg->labels, F, root, flag, labelled);
  launch_exclusive_scan(flag, number, n, tiles, st);      // number[F] = the number of segments
  SMESH_HIP(hipGetLastError());
  uint32_t h_S = 0;
  unsigned long long h_labelled = 0;
  SMESH_HIP(hipMemcpyAsync(&h_S, number + F, 4, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipMemcpyAsync(&h_labelled, labelled, 8, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  sg->S = h_S;
  sg->labelled = h_labelled;
  const uint64_t sbytes = std::max<uint64_t>(sg->S * 4, 16);
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&sg->first_face), sbytes));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&sg->seg_label), sbytes));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&sg->size), sbytes));
  SMESH_HIP(hipMemsetAsync(sg->size, 0, sbytes, st));
  hipLaunchKernelGGL(k_seg_number, gf, b, 0, st, (const uint32_t*)root, (const uint32_t*)number, (const int32_t*)sg->labels, F, sg->ids,
                     sg->first_face, sg->seg_label, sg->size);
  SMESH_HIP(hipGetLastError());
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

// A new handle over the graph's tables; `fill(d_labels)` queues the labels into the handle's own copy.  Context locked, device current.
template <typename Fill>
int create_segments(DeviceCtx* ctx, const uint32_t* offsets, const uint32_t* nbr, uint64_t F, uint64_t nnz,
                    const float* weights, int weights_memkind, float min_weight, smesh_face_segments_t** out, const Fill& fill) {
  smesh_face_segments* sg = new smesh_face_segments;
  sg->ctx = ctx;
  sg->F = F;
  const int status = [&]() -> int {
    SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&sg->labels), std::max<uint64_t>(F * 4, 16)));
    SMESH_TRY(fill(sg->labels));
    TempBlocks tmp;
    const float* d_w = nullptr;
    SMESH_TRY(on_device(ctx, tmp, weights, weights ? nnz * 4 : 0, weights_memkind, &d_w));
    if (weights && nnz == 0) d_w = nullptr;      // (no entry is ever looked at)
    return build_segments(sg, offsets, nbr, d_w, min_weight);
  }();
  if (status != SMESH_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    free_segments(sg);
    return status;
  }
  *out = sg;
  return SMESH_OK;
}

int check_create_args(const smesh_face_graph_t* graph, const float* weights, int weights_memkind, smesh_face_segments_t** out, DeviceCtx** ctx,
                      const uint32_t** offsets, const uint32_t** nbr, uint64_t* F, uint64_t* nnz) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (!graph) return fail(SMESH_ERR_INVALID, "NULL face graph");
  if (weights && !memkind_ok(weights_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  SMESH_TRY(smesh_face_graph_tables(graph, ctx, offsets, nbr, F, nnz));
  if (*F >= 0x80000000ull) return fail(SMESH_ERR_INVALID, "face segments: F must stay below 2^31");
  return SMESH_OK;
}

// The rows form over rows that are on the device already.  Context locked, device current.
int despeckle_device_rows(const smesh_face_segments* sg, DeviceCtx* ctx, uint32_t min_faces, const float* d_rows, uint32_t C, float* out_rows,
                          int out_memkind) {
  hipStream_t st = ctx->stream;
  const uint64_t F = sg->F, elems = F * C;
  if (elems == 0) return SMESH_OK;
  if (div_up(elems, kBlock) > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "face segments: F * C must stay below 2^39");
  TempBlocks tmp;
  Out<float> out;
  SMESH_TRY(out.init(tmp, out_rows, elems * 4, out_memkind));
  float* const d_out = out.dev;
  const bool wide = C % 4 == 0 && (reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_out)) % 16 == 0;
  if (wide)
    hipLaunchKernelGGL(k_seg_despeckle_rows<float4>, grid_for(elems / 4), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(d_rows),
                       (const int32_t*)sg->ids, (const uint32_t*)sg->size, min_faces, elems / 4, C / 4, reinterpret_cast<float4*>(d_out));
  else
    hipLaunchKernelGGL(k_seg_despeckle_rows<float>, grid_for(elems), dim3(kBlock), 0, st, d_rows, (const int32_t*)sg->ids,
                       (const uint32_t*)sg->size, min_faces, elems, C, d_out);
  SMESH_HIP(hipGetLastError());
  SMESH_TRY(out.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

}  // namespace

int smesh_face_segments_tables(smesh_face_segments* sg, SegmentTables* out) {
  if (!sg) return fail(SMESH_ERR_INVALID, "NULL face segments");
  *out = {sg->ctx, sg->F, sg->S, sg->labelled, sg->ids, sg->labels, sg->size, &sg->members};
  return SMESH_OK;
}

extern "C" {

int smesh_face_segments_create(const smesh_face_graph_t* graph, const int32_t* labels, int labels_memkind, const float* weights,
                               int weights_memkind, float min_weight, smesh_face_segments_t** out) {
  DeviceCtx* ctx = nullptr;
  const uint32_t *offsets = nullptr, *nbr = nullptr;
  uint64_t F = 0, nnz = 0;
  SMESH_TRY(check_create_args(graph, weights, weights_memkind, out, &ctx, &offsets, &nbr, &F, &nnz));
  if (!memkind_ok(labels_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  if (F && !labels) return fail(SMESH_ERR_INVALID, "face segments: NULL labels");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  return create_segments(ctx, offsets, nbr, F, nnz, weights, weights_memkind, min_weight, out, [&](int32_t* d_labels) -> int {
    if (F) SMESH_HIP(hipMemcpyAsync(d_labels, labels, F * 4, labels_memkind == SMESH_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    return SMESH_OK;
  });
}

int smesh_aggregator_face_segments(smesh_aggregator_t* ag, const smesh_face_graph_t* graph, float dont_care_threshold, const float* weights,
                                   int weights_memkind, float min_weight, smesh_face_segments_t** out) {
  DeviceCtx* gctx = nullptr;
  const uint32_t *offsets = nullptr, *nbr = nullptr;
  uint64_t F = 0, nnz = 0;
  SMESH_TRY(check_create_args(graph, weights, weights_memkind, out, &gctx, &offsets, &nbr, &F, &nnz));
  if (!ag) return fail(SMESH_ERR_INVALID, "NULL argument");
  return smesh_aggregator_with_final_rows(ag, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("face segments", "face graph", ctx, gctx, P, F));
    return create_segments(ctx, offsets, nbr, F, nnz, weights, weights_memkind, min_weight, out, [&](int32_t* d_labels) -> int {
      if (F == 0) return SMESH_OK;
      // the labels of the finishing step (vertices.hip), written straight into the handle's copy
      return smesh_rows_finish(ctx, d_rows, F, C, SMESH_VTX_ANNOTATIONS, dont_care_threshold, nullptr, d_labels, SMESH_MEM_DEVICE);
    });
  });
}

int smesh_face_segments_destroy(smesh_face_segments_t* sg) {
  if (!sg) return SMESH_OK;
  std::lock_guard<std::recursive_mutex> lock(sg->ctx->mu);
  DeviceScope scope(sg->ctx->device);
  free_segments(sg);
  return SMESH_OK;
}

int smesh_face_segments_size(const smesh_face_segments_t* sg, uint64_t* F, uint64_t* S, uint64_t* labelled) {
  if (!sg) return fail(SMESH_ERR_INVALID, "NULL face segments");
  if (F) *F = sg->F;
  if (S) *S = sg->S;
  if (labelled) *labelled = sg->labelled;
  return SMESH_OK;
}

int smesh_face_segments_get(const smesh_face_segments_t* sg, int32_t* ids, uint32_t* first_face, int32_t* label, uint32_t* size, int out_memkind) {
  if (!sg) return fail(SMESH_ERR_INVALID, "NULL face segments");
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  DeviceCtx* ctx = sg->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  SMESH_TRY(copy_out<int32_t>(ids, sg->ids, sg->F * 4, out_memkind, ctx->stream));
  SMESH_TRY(copy_out<uint32_t>(first_face, sg->first_face, sg->S * 4, out_memkind, ctx->stream));
  SMESH_TRY(copy_out<int32_t>(label, sg->seg_label, sg->S * 4, out_memkind, ctx->stream));
  SMESH_TRY(copy_out<uint32_t>(size, sg->size, sg->S * 4, out_memkind, ctx->stream));
  SMESH_HIP(hipStreamSynchronize(ctx->stream));
  return SMESH_OK;
}

int smesh_face_segments_despeckle_labels(const smesh_face_segments_t* sg, uint32_t min_faces, int32_t* out_labels, int out_memkind,
                                         uint64_t* removed_faces, uint64_t* removed_segments) {
  if (!sg) return fail(SMESH_ERR_INVALID, "NULL face segments");
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  if (sg->F && !out_labels) return fail(SMESH_ERR_INVALID, "face segments: NULL out_labels");
  DeviceCtx* ctx = sg->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  if (removed_faces) *removed_faces = 0;
  if (removed_segments) *removed_segments = 0;
  if (sg->F == 0) return SMESH_OK;
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  Out<int32_t> out;
  unsigned long long* removed = nullptr;      // [0] faces, [1] segments
  SMESH_TRY(out.init(tmp, out_labels, sg->F * 4, out_memkind));
  SMESH_TRY(tmp.alloc(&removed, 16));
  SMESH_HIP(hipMemsetAsync(removed, 0, 16, st));
  hipLaunchKernelGGL(k_seg_despeckle_labels, count_grid(sg->F), dim3(kBlock), 0, st, (const int32_t*)sg->labels, (const int32_t*)sg->ids,
                     (const uint32_t*)sg->size, min_faces, sg->F, out.dev, removed);
  if (removed_segments && sg->S)
    hipLaunchKernelGGL(k_seg_small, count_grid(sg->S), dim3(kBlock), 0, st, (const uint32_t*)sg->size, min_faces, sg->S, removed + 1);
  SMESH_HIP(hipGetLastError());
  unsigned long long h_removed[2] = {0, 0};
  SMESH_HIP(hipMemcpyAsync(h_removed, removed, 16, hipMemcpyDeviceToHost, st));
  SMESH_TRY(out.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (removed_faces) *removed_faces = h_removed[0];
  if (removed_segments) *removed_segments = h_removed[1];
  return SMESH_OK;
}

int smesh_face_segments_despeckle_rows(const smesh_face_segments_t* sg, uint32_t min_faces, const float* rows, int rows_memkind, uint32_t C,
                                       float* out_rows, int out_memkind) {
  if (!sg) return fail(SMESH_ERR_INVALID, "NULL face segments");
  if (C == 0) return fail(SMESH_ERR_INVALID, "face segments: the class count must be positive");
  if (!memkind_ok(rows_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  if (sg->F && (!rows || !out_rows)) return fail(SMESH_ERR_INVALID, "face segments: NULL rows");
  DeviceCtx* ctx = sg->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(ctx, tmp, rows, (size_t)sg->F * C * 4, rows_memkind, &d_rows));
  return despeckle_device_rows(sg, ctx, min_faces, d_rows, C, out_rows, out_memkind);
}

int smesh_aggregator_face_segments_despeckle(smesh_aggregator_t* ag, const smesh_face_segments_t* sg, uint32_t min_faces, float* out_rows,
                                             int out_memkind) {
  if (!ag || !sg) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "face segments: bad memory kind");
  if (sg->F && !out_rows) return fail(SMESH_ERR_INVALID, "face segments: NULL out_rows");
  return smesh_aggregator_with_final_rows(ag, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("face segments", "segments", ctx, sg->ctx, P, sg->F));
    return despeckle_device_rows(sg, ctx, min_faces, d_rows, C, out_rows, out_memkind);
  });
}

}  // extern "C"
