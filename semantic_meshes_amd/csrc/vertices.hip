// vertices.hip -- per-vertex results (include/smesh_vertices.h): the vertex-to-faces CSR of a mesh, built on the device, and the
// gather-and-reduce over the [F, C] face rows that turns face annotations into vertex annotations and labels.
//
// Reference: eval-scannet/eval_scannet.py:249-287 -- a Python loop over every face into a list of sets (:255-258), tf.gather +
// reduce_sum per vertex, "don't care" below 0.9, renormalise.
//
// The sums are defined to the bit (smesh_vertices.h): ONE lane owns one (vertex, class) sum and adds the vertex's face rows in
// ascending face order, so no float atomics anywhere and the result does not depend on how the lists were filled (they are sorted).
#include "mesh_host.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smesh_vertices.h"

using namespace smesh;

struct smesh_vertex_map {
  DeviceCtx* ctx = nullptr;
  uint64_t F = 0, V = 0, nnz = 0;
  uint32_t* offsets = nullptr;   // [V + 1]
  uint32_t* list = nullptr;      // [nnz] faces of vertex v: list[offsets[v] .. offsets[v + 1]), ascending
};

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;

// ---- building the CSR ----------------------------------------------------------------------------------------------------------
// The reference's set per vertex (:255-258): a face that names a vertex twice is one entry of that vertex's list.
__device__ __forceinline__ int distinct_corners(int a, int b, int c, int out[3]) {
  int n = 0;
  out[n++] = a;
  if (b != a) out[n++] = b;
  if (c != a && c != b) out[n++] = c;
  return n;
}

__global__ __launch_bounds__(kBlock) void k_vtx_count(const int32_t* __restrict__ faces, uint64_t F, uint64_t V, uint32_t* __restrict__ count,
                                                      uint32_t* __restrict__ bad) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (a < 0 || b < 0 || c < 0 || (uint64_t)a >= V || (uint64_t)b >= V || (uint64_t)c >= V) {
    atomicOr(bad, 1u);
    return;
  }
  int v[3];
  const int n = distinct_corners(a, b, c, v);
  for (int i = 0; i < n; i++) atomicAdd(&count[v[i]], 1u);
}

#include "scan.inc.hpp"   // k_scan_tiles, k_scan_sums, k_scan_add

// `cursor` is all zero: the order in which the faces of a vertex arrive is whatever the atomics make it -- the sort below undoes it.
__global__ __launch_bounds__(kBlock) void k_vtx_fill(const int32_t* __restrict__ faces, uint64_t F, const uint32_t* __restrict__ offsets,
                                                     uint32_t* __restrict__ cursor, uint32_t* __restrict__ list) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int v[3];
  const int n = distinct_corners(faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2], v);
  for (int i = 0; i < n; i++) list[offsets[v[i]] + atomicAdd(&cursor[v[i]], 1u)] = (uint32_t)f;
}

// Lists of up to kShortList faces (a manifold mesh: about six) are sorted by their vertex's thread, in place; longer ones are queued
// for k_vtx_sort_long.  At most nnz / (kShortList + 1) vertices can be queued.
constexpr uint32_t kShortList = 32;

__global__ __launch_bounds__(kBlock) void k_vtx_sort_short(const uint32_t* __restrict__ offsets, uint64_t V, uint32_t* __restrict__ list,
                                                           uint32_t* __restrict__ queue, uint32_t* __restrict__ queue_len) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  const uint32_t beg = offsets[v], n = offsets[v + 1] - beg;
  if (n < 2) return;
  if (n > kShortList) {
    queue[atomicAdd(queue_len, 1u)] = (uint32_t)v;
    return;
  }
  uint32_t* const l = list + beg;
  for (uint32_t i = 1; i < n; i++) {
    const uint32_t x = l[i];
    uint32_t j = i;
    for (; j > 0 && l[j - 1] > x; j--) l[j] = l[j - 1];
    l[j] = x;
  }
}

// A list of ANY length: one workgroup runs a bitonic network over it in global memory.  Every comparator puts the smaller value at
// the lower position (the first stage of each merge pairs i with its mirror image in the block), so a list whose length is not a
// power of two needs no padding in memory: positions from n on stand for +inf, and a comparator that touches one never swaps.
__global__ __launch_bounds__(kBlock) void k_vtx_sort_long(const uint32_t* __restrict__ offsets, uint32_t* list,
                                                          const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queue_len) {
  const uint32_t qn = *queue_len;
  for (uint32_t q = blockIdx.x; q < qn; q += gridDim.x) {
    const uint32_t v = queue[q];
    const uint32_t beg = offsets[v], n = offsets[v + 1] - beg;
    uint32_t* const l = list + beg;
    uint64_t npad = 1;
    while (npad < n) npad <<= 1;
    const uint64_t half = npad >> 1;
    for (uint64_t k = 2; k <= npad; k <<= 1) {
      for (uint64_t j = k >> 1; j > 0; j >>= 1) {
        const bool mirror = j == (k >> 1);
        for (uint64_t i = threadIdx.x; i < half; i += kBlock) {
          const uint64_t lo = 2 * j * (i / j) + i % j;
          const uint64_t hi = mirror ? 2 * j * (i / j) + (k - 1 - i % j) : lo + j;
          if (hi < n) {
            const uint32_t a = l[lo], b = l[hi];
            if (a > b) { l[lo] = b; l[hi] = a; }
          }
        }
        __syncthreads();
      }
    }
  }
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------
struct GatherArgs {
  // items: the vertices of a map (offsets + list name the rows of each), the faces of a texel layout (list == nullptr: item i owns
  // the rows [seg_first[i], seg_first[i] + seg_res[i] (seg_res[i] + 1) / 2)) or the rows themselves (neither: item i owns row i)
  const uint32_t* offsets;
  const uint32_t* list;
  const uint32_t* seg_first;
  const uint32_t* seg_res;
  const float* rows;      // [.., C] the rows that are summed
  uint64_t n;             // items
  uint32_t C;
  int mode;
  float threshold;
  float* out_rows;        // [n, C] or null
  int32_t* out_labels;    // [n] or null
};

// A group of G lanes owns one item; lane l of the group owns the classes l, l + G, ... (NCH of them; G < 64 only with NCH == 1: rows
// of up to 64 classes, several items per wave so that lanes are not idle on a 19-float row).  Wider rows take a wave per item and
// walk the classes in coalesced chunks of 64.  NCH == 0: any class count -- chunk after chunk with the sums written out as they
// are complete and, for annotations, divided by the row total in a second pass of the same lanes over their own elements.
template <int G, int NCH>
__global__ __launch_bounds__(kBlock) void k_vertex_gather(GatherArgs a) {
  static_assert(G == kWave || NCH == 1, "narrow groups hold one class per lane");
  constexpr int R = NCH > 0 ? NCH : 1;
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t item = tid / G;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int gl = lane & (G - 1);          // lane within the group
  const int gbase = lane - gl;            // first lane of the group within the wave
  const bool valid = item < a.n;          // (a whole group at a time: nobody leaves before the cross-lane steps)
  const uint32_t C = a.C;

  uint32_t beg = 0, end = 0;
  if (valid) {
    if (a.list) { beg = a.offsets[item]; end = a.offsets[item + 1]; }
    else if (a.seg_first) { const uint32_t r = a.seg_res[item]; beg = a.seg_first[item]; end = beg + r * (r + 1) / 2; }
    else { beg = (uint32_t)item; end = beg + 1u; }
  }
  const uint32_t* const list = a.list;
  const float* const rows = a.rows;
  const uint32_t chunks = NCH > 0 ? (uint32_t)NCH : (C + G - 1) / G;
  const bool need_total = a.out_labels != nullptr || a.mode != SMESH_VTX_SUMS;   // (plain sums: no cross-lane step at all)

  float total = 0.0f;            // the row total, added in ascending c: identical in every lane of the group
  float best = 0.0f;             // this lane's largest sum and its class (lowest class first)
  int best_c = 0x7FFFFFFF;
  float s[R];

  for (uint32_t ch0 = 0; ch0 < chunks; ch0 += R) {
    for (int j = 0; j < R; j++) s[j] = 0.0f;
    // the sums: four rows in flight, added one after another in list order
    uint32_t k = beg;
    for (; k + 4 <= end; k += 4) {
      uint64_t r0, r1, r2, r3;
      if (list) { r0 = list[k]; r1 = list[k + 1]; r2 = list[k + 2]; r3 = list[k + 3]; }
      else { r0 = k; r1 = k + 1; r2 = k + 2; r3 = k + 3; }
      float x0[R], x1[R], x2[R], x3[R];
#pragma unroll
      for (int j = 0; j < R; j++) {
        const uint32_t c = (ch0 + j) * G + gl;
        const bool on = c < C;
        x0[j] = on ? rows[r0 * C + c] : 0.0f;
        x1[j] = on ? rows[r1 * C + c] : 0.0f;
        x2[j] = on ? rows[r2 * C + c] : 0.0f;
        x3[j] = on ? rows[r3 * C + c] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < R; j++) { s[j] += x0[j]; s[j] += x1[j]; s[j] += x2[j]; s[j] += x3[j]; }
    }
    for (; k < end; k++) {
      const uint64_t r = list ? list[k] : k;
#pragma unroll
      for (int j = 0; j < R; j++) {
        const uint32_t c = (ch0 + j) * G + gl;
        if (c < C) s[j] += rows[r * C + c];
      }
    }
    // the row total in ascending class order, and this lane's candidates for the label.  Every lane of the group adds the same
    // `width` values in the same order (one cross-lane read each), so all of them hold the total for the division below.  What these
    // serial reads cost beside the memory traffic has NOT been measured (tools/vertex_transfer_bench.py reports the kernel as a whole);
    // neither has the choice to keep up to kMaxRegisterChunks chunks of sums in registers against the chunk-by-chunk form (NCH == 0).
#pragma unroll
    for (int j = 0; j < R; j++) {
      const uint32_t c0 = (ch0 + j) * G;
      const int width = (int)min((uint32_t)G, C > c0 ? C - c0 : 0u);
      if (G == 1) {
        if (width) total += s[j];
      } else if (need_total) {
        for (int l = 0; l < width; l++) total += __shfl(s[j], gbase + l, kWave);
      }
      const uint32_t c = c0 + gl;
      if (c < C && (best_c == 0x7FFFFFFF || s[j] > best)) { best = s[j]; best_c = (int)c; }
    }
    if (NCH == 0 && a.out_rows && valid) {
      const uint32_t c = ch0 * G + gl;
      if (c < C) a.out_rows[item * C + c] = s[0];
    }
  }

  const bool dont_care = beg == end || total < a.threshold;   // (nothing to sum: don't care whatever the threshold, zero and negative ones included)
  if (a.out_labels) {
    // the largest sum of the group, the lowest class among equals
#pragma unroll
    for (int d = G >> 1; d > 0; d >>= 1) {
      const float ob = __shfl_xor(best, d, kWave);
      const int oc = __shfl_xor(best_c, d, kWave);
      if (oc != 0x7FFFFFFF && (best_c == 0x7FFFFFFF || ob > best || (ob == best && oc < best_c))) { best = ob; best_c = oc; }
    }
    if (valid && gl == 0) a.out_labels[item] = dont_care ? -1 : best_c;
  }
  if (a.out_rows && valid) {
    if (NCH > 0) {
#pragma unroll
      for (int j = 0; j < R; j++) {
        const uint32_t c = (uint32_t)j * G + gl;
        if (c < C) a.out_rows[item * C + c] = a.mode == SMESH_VTX_SUMS ? s[j] : dont_care ? 0.0f : s[j] / total;
      }
    } else if (a.mode != SMESH_VTX_SUMS) {
      for (uint32_t c = gl; c < C; c += G) {      // (the elements this lane wrote above)
        float* const p = a.out_rows + item * C + c;
        *p = dont_care ? 0.0f : *p / total;
      }
    }
  }
}

template <int G, int NCH>
void launch_one(const GatherArgs& a, hipStream_t st) {
  const uint64_t threads = a.n * G;
  hipLaunchKernelGGL((k_vertex_gather<G, NCH>), dim3((uint32_t)div_up(threads, kBlock)), dim3(kBlock), 0, st, a);
}

constexpr uint32_t kMaxRegisterChunks = 8;   // rows of up to 512 classes keep their sums in registers

int launch_gather(DeviceCtx* ctx, const GatherArgs& a) {
  if (a.n == 0) return SMESH_OK;
  if (a.n * 64 / kBlock >= 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "vertex gather: too many rows for one launch");
  hipStream_t st = ctx->stream;
  const uint32_t C = a.C;
  if (C <= 1) launch_one<1, 1>(a, st);
  else if (C <= 2) launch_one<2, 1>(a, st);
  else if (C <= 4) launch_one<4, 1>(a, st);
  else if (C <= 8) launch_one<8, 1>(a, st);
  else if (C <= 16) launch_one<16, 1>(a, st);
  else if (C <= 32) launch_one<32, 1>(a, st);
  else {
    switch (div_up(C, kWave) <= kMaxRegisterChunks ? (int)div_up(C, kWave) : 0) {
      case 1: launch_one<kWave, 1>(a, st); break;
      case 2: launch_one<kWave, 2>(a, st); break;
      case 3: launch_one<kWave, 3>(a, st); break;
      case 4: launch_one<kWave, 4>(a, st); break;
      case 5: launch_one<kWave, 5>(a, st); break;
      case 6: launch_one<kWave, 6>(a, st); break;
      case 7: launch_one<kWave, 7>(a, st); break;
      case 8: launch_one<kWave, 8>(a, st); break;
      default: launch_one<kWave, 0>(a, st); break;
    }
  }
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// The gather over rows that are on the device already; the outputs go where the caller wants them.  Context locked, device current.
int gather_device_rows(DeviceCtx* ctx, GatherArgs a, float* out_rows, int32_t* out_labels, int out_memkind) {
  TempBlocks tmp;
  Out<float> rows;
  Out<int32_t> labels;
  SMESH_TRY(rows.init(tmp, out_rows, (size_t)a.n * a.C * 4, out_memkind));
  SMESH_TRY(labels.init(tmp, out_labels, (size_t)a.n * 4, out_memkind));
  a.out_rows = rows.dev;
  a.out_labels = labels.dev;
  SMESH_TRY(launch_gather(ctx, a));
  SMESH_TRY(rows.copy_back(ctx->stream));
  SMESH_TRY(labels.copy_back(ctx->stream));
  SMESH_HIP(hipStreamSynchronize(ctx->stream));
  return SMESH_OK;
}

GatherArgs map_args(const smesh_vertex_map* m, const float* d_rows, uint32_t C, int mode, float threshold) {
  GatherArgs a = {};
  a.offsets = m->offsets;
  a.list = m->list;
  a.rows = d_rows;
  a.n = m->V;
  a.C = C;
  a.mode = mode;
  a.threshold = threshold;
  return a;
}

int build_map(smesh_vertex_map* m, const int32_t* faces) {
  DeviceCtx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t F = m->F, V = m->V, n = V + 1;
  TempBlocks tmp;
  int32_t* d_faces = nullptr;
  uint32_t *count = nullptr, *tiles = nullptr, *flags = nullptr, *queue = nullptr;   // flags: [0] bad index seen, [1] queue length
  const uint64_t ntiles = div_up(n, kScanTile), queue_cap = 3 * F / (kShortList + 1) + 1;
  SMESH_TRY(tmp.alloc(&d_faces, F * 12));
  SMESH_TRY(tmp.alloc(&count, n * 4));
  SMESH_TRY(tmp.alloc(&tiles, ntiles * 4));
  SMESH_TRY(tmp.alloc(&flags, 16));
  SMESH_TRY(tmp.alloc(&queue, queue_cap * 4));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->offsets), std::max<uint64_t>(n * 4, 16)));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->list), std::max<uint64_t>(3 * F * 4, 16)));
  SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));
  SMESH_HIP(hipMemsetAsync(flags, 0, 16, st));
  const dim3 gf((uint32_t)div_up(F, kBlock)), gv((uint32_t)div_up(V, kBlock)), b(kBlock);
  if (F) {
    SMESH_HIP(hipMemcpyAsync(d_faces, faces, F * 12, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_vtx_count, gf, b, 0, st, d_faces, F, V, count, flags);
  }
  // offsets = exclusive scan of count[0 .. V] (count[V] == 0, so offsets[V] is the number of entries)
  launch_exclusive_scan(count, m->offsets, n, tiles, st);
  SMESH_HIP(hipGetLastError());
  uint32_t h_flags[4] = {0, 0, 0, 0}, h_nnz = 0;
  SMESH_HIP(hipMemcpyAsync(h_flags, flags, 16, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipMemcpyAsync(&h_nnz, m->offsets + V, 4, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (h_flags[0]) return fail(SMESH_ERR_INVALID, "vertex map: a face index lies outside [0, " + std::to_string(V) + ")");
  m->nnz = h_nnz;
  if (F && V) {
    SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));      // now the fill cursors
    hipLaunchKernelGGL(k_vtx_fill, gf, b, 0, st, d_faces, F, m->offsets, count, m->list);
    hipLaunchKernelGGL(k_vtx_sort_short, gv, b, 0, st, m->offsets, V, m->list, queue, flags + 1);
    hipLaunchKernelGGL(k_vtx_sort_long, dim3((uint32_t)std::min<uint64_t>(queue_cap, 1024)), b, 0, st, m->offsets, m->list, queue, flags + 1);
    SMESH_HIP(hipGetLastError());
  }
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

}  // namespace

// What eval.hip (smesh_aggregator_labels) needs: the label of every row of a dense float32 [n, C] array on the device -- a vertex
// that owns exactly one row: 0 + x == x, so the row total and the label are those of the row itself.  Context locked, device current.
int smesh_rows_labels(DeviceCtx* ctx, const float* d_rows, uint64_t n, uint32_t C, float dont_care_threshold, int32_t* out_labels, int out_memkind) {
  SMESH_TRY(check_gather_args("vertex gather", C, SMESH_VTX_ANNOTATIONS, nullptr, out_labels, SMESH_MEM_DEVICE, out_memkind));
  if (n >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "labels: the row count must stay below 2^32");
  GatherArgs g = {};
  g.rows = d_rows;
  g.n = n;
  g.C = C;
  g.mode = SMESH_VTX_ANNOTATIONS;
  g.threshold = dont_care_threshold;
  return gather_device_rows(ctx, g, nullptr, out_labels, out_memkind);
}

// What face_graph.hip needs: the same gather with rows and/or labels out, and the device CSR of a map.
int smesh_rows_finish(DeviceCtx* ctx, const float* d_rows, uint64_t n, uint32_t C, int mode, float dont_care_threshold, float* out_rows,
                      int32_t* out_labels, int out_memkind) {
  SMESH_TRY(check_gather_args("vertex gather", C, mode, out_rows, out_labels, SMESH_MEM_DEVICE, out_memkind));
  if (n >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "rows: the row count must stay below 2^32");
  GatherArgs g = {};
  g.rows = d_rows;
  g.n = n;
  g.C = C;
  g.mode = mode;
  g.threshold = dont_care_threshold;
  return gather_device_rows(ctx, g, out_rows, out_labels, out_memkind);
}

int smesh_vertex_map_tables(const smesh_vertex_map* m, DeviceCtx** ctx, const uint32_t** offsets, const uint32_t** list) {
  if (!m) return fail(SMESH_ERR_INVALID, "NULL vertex map");
  *ctx = m->ctx;
  *offsets = m->offsets;
  *list = m->list;
  return SMESH_OK;
}

extern "C" {

int smesh_vertex_map_create(const int32_t* faces, uint64_t F, uint64_t V, int device, smesh_vertex_map_t** out) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (F && !faces) return fail(SMESH_ERR_INVALID, "vertex map: NULL faces");
  if (3 * F >= 0xFFFFFFFFull || V >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "vertex map: 3 F and V must stay below 2^32");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  smesh_vertex_map* m = new smesh_vertex_map;
  m->ctx = ctx;
  m->F = F;
  m->V = V;
  const int status = build_map(m, faces);
  if (status != SMESH_OK) {
    smesh_vertex_map_destroy(m);
    return status;
  }
  *out = m;
  return SMESH_OK;
}

int smesh_vertex_map_destroy(smesh_vertex_map_t* m) {
  if (!m) return SMESH_OK;
  std::lock_guard<std::recursive_mutex> lock(m->ctx->mu);
  DeviceScope scope(m->ctx->device);
  if (m->offsets) (void)dev_free(m->offsets);
  if (m->list) (void)dev_free(m->list);
  delete m;
  return SMESH_OK;
}

int smesh_vertex_map_size(const smesh_vertex_map_t* m, uint64_t* F, uint64_t* V, uint64_t* nnz) {
  if (!m) return fail(SMESH_ERR_INVALID, "NULL vertex map");
  if (F) *F = m->F;
  if (V) *V = m->V;
  if (nnz) *nnz = m->nnz;
  return SMESH_OK;
}

int smesh_vertex_map_adjacency(const smesh_vertex_map_t* m, uint64_t* offsets, uint32_t* faces) {
  if (!m || !offsets || (m->nnz && !faces)) return fail(SMESH_ERR_INVALID, "NULL argument");
  return csr_to_host(m->ctx, m->offsets, m->V, m->list, m->nnz, offsets, faces);
}

int smesh_vertex_map_gather(const smesh_vertex_map_t* m, const float* face_rows, int rows_memkind, uint32_t C, int mode,
                            float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  if (!m) return fail(SMESH_ERR_INVALID, "NULL vertex map");
  SMESH_TRY(check_gather_args("vertex gather", C, mode, out_rows, out_labels, rows_memkind, out_memkind));
  if (m->F && !face_rows) return fail(SMESH_ERR_INVALID, "vertex gather: NULL face rows");
  DeviceCtx* ctx = m->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(ctx, tmp, face_rows, (size_t)m->F * C * 4, rows_memkind, &d_rows));
  return gather_device_rows(ctx, map_args(m, d_rows, C, mode, dont_care_threshold), out_rows, out_labels, out_memkind);
}

int smesh_aggregator_vertex_annotations(smesh_aggregator_t* a, const smesh_vertex_map_t* m, int mode, float dont_care_threshold,
                                        float* out_rows, int32_t* out_labels, int out_memkind) {
  if (!a || !m) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(check_gather_args("vertex gather", 1, mode, out_rows, out_labels, SMESH_MEM_DEVICE, out_memkind));
  return smesh_aggregator_with_final_rows(a, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("vertex annotations", "vertex map", ctx, m->ctx, P, m->F));
    return gather_device_rows(ctx, map_args(m, d_rows, C, mode, dont_care_threshold), out_rows, out_labels, out_memkind);
  });
}

int smesh_renderer_texel_face_rows(smesh_renderer_t* r, const float* texel_rows, int rows_memkind, uint32_t C, int mode,
                                   float dont_care_threshold, float* out_face_rows, int out_memkind) {
  if (!r) return fail(SMESH_ERR_INVALID, "NULL renderer");
  SMESH_TRY(check_gather_args("vertex gather", C, mode, out_face_rows, nullptr, rows_memkind, out_memkind));
  DeviceCtx* ctx = nullptr;
  uint64_t F = 0, P = 0;
  GatherArgs g = {};
  SMESH_TRY(smesh_renderer_texel_tables(r, &ctx, &F, &P, &g.seg_first, &g.seg_res));
  if (P && !texel_rows) return fail(SMESH_ERR_INVALID, "texel face rows: NULL texel rows");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  TempBlocks tmp;
  SMESH_TRY(on_device(ctx, tmp, texel_rows, (size_t)P * C * 4, rows_memkind, &g.rows));
  g.n = F;
  g.C = C;
  g.mode = mode;
  g.threshold = dont_care_threshold;
  return gather_device_rows(ctx, g, out_face_rows, nullptr, out_memkind);
}

}  // extern "C"
