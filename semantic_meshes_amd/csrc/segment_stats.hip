// segment_stats.hip -- fused votes and areas pooled over the segments of a labelled mesh (include/smesh_segment_stats.h): the member
// table of the segments of face_segments.hip, the ordered float reduction over it, its broadcast back to the faces, face areas, and
// the despeckle by a per-segment measure.
//
// The reference has no such step.  Every float result is defined to the bit by the header's rule, so this file is written around
// three rules of its own.
//
//   1. No atomics decide a position or a sum.  The member table is a stable sort of the labelled faces by segment id: a compaction
//      by scan (ascending f), then an LSD radix sort over the ceil(log2 S) bits of the id whose every pass is a stable split (count,
//      scan, scatter), four bits at a time or one.  The sums are serial inside a chunk of 256 members and serial over a segment's
//      chunks; what runs in parallel is chunks, segments and classes.
//   2. The launch sequence is fixed by F and S alone: the split passes, one chunk launch, one launch over the segments with more
//      than one chunk.  There is no "until nothing changed".
//   3. Nobody waits.  No grid barrier, no cooperative launch, no polling; every loop has a trip count that is known when its kernel
//      is launched (stated at each).
#include "mesh_host.hpp"

#include <algorithm>
#include <string>

#include "../../include/smesh_segment_stats.h"

using namespace smesh;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr uint32_t kChunk = 256;      // the members of one chunk sum (the header's rule)
constexpr int kInFlight = 8;          // rows whose loads are issued before the first of them is added

#include "scan.inc.hpp"    // launch_exclusive_scan
#include "count.inc.hpp"   // kCountBlocks, block_count_add, count_grid

dim3 grid_for(uint64_t n) { return dim3((uint32_t)div_up(n, kBlock)); }

// ---- the member table -----------------------------------------------------------------------------------------------------------
// flag[f] = 1 for a labelled face, flag[F] = 0: the exclusive scan over F + 1 elements gives every labelled face its place among
// the labelled faces, ascending.
__global__ __launch_bounds__(kBlock) void k_ss_labelled(const int32_t* __restrict__ ids, uint64_t F, uint32_t* __restrict__ flag) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f <= F) flag[f] = f < F && ids[f] >= 0 ? 1u : 0u;
}

// place[f] < labelled for every labelled face (the scan of the flags above), so every store lands inside out[labelled].
__global__ __launch_bounds__(kBlock) void k_ss_compact(const int32_t* __restrict__ ids, const uint32_t* __restrict__ place, uint64_t F,
                                                       uint32_t* __restrict__ out) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f < F && ids[f] >= 0) out[place[f]] = (uint32_t)f;
}

// One stable split by bit `bit` of the segment id.  flag[i] = 1 where the bit of src[i]'s id is clear, flag[L] = 0.
__global__ __launch_bounds__(kBlock) void k_ss_bit_flag(const uint32_t* __restrict__ src, const int32_t* __restrict__ ids, uint64_t L, int bit,
                                                        uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i <= L) flag[i] = i < L && (((uint32_t)ids[src[i]] >> bit) & 1u) == 0u ? 1u : 0u;
}

// clear[i] = the faces before i whose bit is clear, clear[L] = all of them.  A face with a clear bit goes to clear[i]; one with a
// set bit goes behind all of those, to clear[L] + (i - clear[i]).  Both are below L: the first because clear[i] counts faces other
// than i among the clear[L] clear ones, the second because i - clear[i] counts faces other than i among the L - clear[L] set ones.
__global__ __launch_bounds__(kBlock) void k_ss_bit_scatter(const uint32_t* __restrict__ src, const int32_t* __restrict__ ids,
                                                           const uint32_t* __restrict__ clear, uint64_t L, int bit, uint32_t* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= L) return;
  const uint32_t f = src[i], before = clear[i];
  const bool set = (((uint32_t)ids[f] >> bit) & 1u) != 0u;
  dst[set ? clear[L] + ((uint32_t)i - before) : before] = f;
}

// The same split by a digit of `bits` bits (D = 1 << bits values, at most kMaxDigit) in two launches around one short scan: a tile is
// the kBlock faces of one workgroup.  A face's rank among the tile's faces with its digit comes from ballots -- the lanes before it
// in its wave, then the waves before its wave -- so the order inside a digit is the order of the input: stable, no atomics.
// counts[d * tiles + tile] in digit-major order makes the exclusive scan of counts the place of every (digit, tile) run.
constexpr int kMaxDigitBits = 4, kMaxDigit = 1 << kMaxDigitBits;

// The ballots of one tile: this lane's rank inside its wave among the lanes with its digit; wave_count[w][d] once the barrier is passed.
// The loop runs D turns for every lane.
__device__ __forceinline__ uint32_t tile_digit_rank(bool valid, uint32_t digit, int D, uint32_t (*wave_count)[kMaxDigit]) {
  const int lane = (int)(threadIdx.x & (kWave - 1)), wave = (int)(threadIdx.x / kWave);
  unsigned long long mine = 0;
  for (int d = 0; d < D; d++) {
    const unsigned long long mask = __ballot(valid && digit == (uint32_t)d);
    if (digit == (uint32_t)d) mine = mask;
    if (lane == 0) wave_count[wave][d] = (uint32_t)__popcll(mask);
  }
  __syncthreads();
  return (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void k_ss_digit_count(const uint32_t* __restrict__ src, const int32_t* __restrict__ ids, uint64_t L, int shift,
                                                           int bits, uint32_t tiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_count[kBlock / kWave][kMaxDigit];
  const int D = 1 << bits;
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < L;
  const uint32_t digit = valid ? ((uint32_t)ids[src[i]] >> shift) & (uint32_t)(D - 1) : 0u;
  (void)tile_digit_rank(valid, digit, D, wave_count);
  if ((int)threadIdx.x < D) {
    uint32_t n = 0;
    for (int w = 0; w < kBlock / kWave; w++) n += wave_count[w][threadIdx.x];
    counts[(uint64_t)threadIdx.x * tiles + blockIdx.x] = n;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x == D) counts[(uint64_t)D * tiles] = 0u;      // (the scan's last element: the total)
}

// place[d * tiles + tile] counts the faces with a lower digit and those with digit d in earlier tiles; the faces of this tile with
// digit d in earlier waves and earlier lanes come on top.  Every term counts faces other than this one, so the sum is below L.
__global__ __launch_bounds__(kBlock) void k_ss_digit_scatter(const uint32_t* __restrict__ src, const int32_t* __restrict__ ids, uint64_t L, int shift,
                                                             int bits, uint32_t tiles, const uint32_t* __restrict__ place,
                                                             uint32_t* __restrict__ dst) {
  __shared__ uint32_t wave_count[kBlock / kWave][kMaxDigit];
  const int D = 1 << bits;
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < L;
  const uint32_t f = valid ? src[i] : 0u;
  const uint32_t digit = valid ? ((uint32_t)ids[f] >> shift) & (uint32_t)(D - 1) : 0u;
  uint32_t at = tile_digit_rank(valid, digit, D, wave_count);
  for (int w = 0; w < (int)(threadIdx.x / kWave); w++) at += wave_count[w][digit];      // (at most three turns)
  if (valid) dst[place[(uint64_t)digit * tiles + blockIdx.x] + at] = f;
}

// What the three scans over S + 1 elements start from: the size, the chunks, and the chunks of segments with more than one.
__global__ __launch_bounds__(kBlock) void k_ss_counts(const uint32_t* __restrict__ size, uint64_t S, uint32_t* __restrict__ padded,
                                                      uint32_t* __restrict__ chunks, uint32_t* __restrict__ partials) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s > S) return;
  const uint32_t n = s < S ? size[s] : 0u, c = n / kChunk + (n % kChunk ? 1u : 0u);
  padded[s] = n;
  chunks[s] = c;
  partials[s] = c > 1 ? c : 0u;
}

// The digit width of the member table's sort.  Same results either way; SMESH_SEGMENT_SORT_BITS (1 .. kMaxDigitBits, read at every
// build) is what tools/segment_stats_bench.py alternates to compare the widths, and what the tests set to run both forms.
// Four bits: measured on the 1 M-triangle mesh against the one-bit split in three alternating rounds, 0.19 against 0.33 ms at 512
// segments (9 bits) and 0.21 against 0.48 ms at 28 778 (15 bits), outside the repeats' min - max every time.
constexpr int kSortDigitBits = 4;
int sort_digit_bits() { return std::min(std::max(env_int("SMESH_SEGMENT_SORT_BITS", kSortDigitBits), 1), kMaxDigitBits); }

void release_members(SegmentMembers* m) {
  for (uint32_t** p : {&m->offsets, &m->members, &m->chunk_start, &m->partial_start}) {
    if (*p) (void)dev_free(*p);
    *p = nullptr;
  }
}

int build_members(const SegmentTables& t) {
  SegmentMembers* m = t.members;
  hipStream_t st = t.ctx->stream;
  const uint64_t F = t.F, S = t.S, L = t.labelled, sort_tiles = div_up(L, kBlock);
  const uint64_t n = std::max(std::max(F, S), kMaxDigit * sort_tiles) + 1;      // what the longest scan takes
  const int digit_bits = sort_digit_bits();
  TempBlocks tmp;
  uint32_t *flag = nullptr, *place = nullptr, *tiles = nullptr, *other = nullptr, *padded = nullptr, *chunks = nullptr, *partials = nullptr;
  SMESH_TRY(tmp.alloc(&flag, n * 4));
  SMESH_TRY(tmp.alloc(&place, n * 4));
  SMESH_TRY(tmp.alloc(&tiles, div_up(n, kScanTile) * 4));
  SMESH_TRY(tmp.alloc(&other, L * 4));
  SMESH_TRY(tmp.alloc(&padded, (S + 1) * 4));
  SMESH_TRY(tmp.alloc(&chunks, (S + 1) * 4));
  SMESH_TRY(tmp.alloc(&partials, (S + 1) * 4));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->offsets), (S + 1) * 4 + 16));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->members), L * 4 + 16));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->chunk_start), (S + 1) * 4 + 16));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&m->partial_start), (S + 1) * 4 + 16));
  const dim3 b(kBlock);
  hipLaunchKernelGGL(k_ss_counts, grid_for(S + 1), b, 0, st, t.size, S, padded, chunks, partials);
  launch_exclusive_scan(padded, m->offsets, S + 1, tiles, st);
  launch_exclusive_scan(chunks, m->chunk_start, S + 1, tiles, st);
  launch_exclusive_scan(partials, m->partial_start, S + 1, tiles, st);
  if (L) {
    // the bits that tell S ids apart; S <= 1 needs no pass.  An even number of passes starts in the handle's array, an odd number
    // in the other one, so that the last pass ends in the handle's.
    int bits = 0;
    while (S > 1 && ((S - 1) >> bits) != 0) bits++;
    const int passes = (bits + digit_bits - 1) / digit_bits;
    uint32_t *src = passes % 2 ? other : m->members, *dst = passes % 2 ? m->members : other;
    hipLaunchKernelGGL(k_ss_labelled, grid_for(F + 1), b, 0, st, t.ids, F, flag);
    launch_exclusive_scan(flag, place, F + 1, tiles, st);
    hipLaunchKernelGGL(k_ss_compact, grid_for(F), b, 0, st, t.ids, (const uint32_t*)place, F, src);
    for (int shift = 0; shift < bits; shift += digit_bits) {      // fixed by S alone
      const int width = std::min(digit_bits, bits - shift);
      if (digit_bits == 1) {
        hipLaunchKernelGGL(k_ss_bit_flag, grid_for(L + 1), b, 0, st, (const uint32_t*)src, t.ids, L, shift, flag);
        launch_exclusive_scan(flag, place, L + 1, tiles, st);
        hipLaunchKernelGGL(k_ss_bit_scatter, grid_for(L), b, 0, st, (const uint32_t*)src, t.ids, (const uint32_t*)place, L, shift, dst);
      } else {
        const dim3 g((uint32_t)sort_tiles);
        hipLaunchKernelGGL(k_ss_digit_count, g, b, 0, st, (const uint32_t*)src, t.ids, L, shift, width, (uint32_t)sort_tiles, flag);
        launch_exclusive_scan(flag, place, ((uint64_t)sort_tiles << width) + 1, tiles, st);
        hipLaunchKernelGGL(k_ss_digit_scatter, g, b, 0, st, (const uint32_t*)src, t.ids, L, shift, width, (uint32_t)sort_tiles, (const uint32_t*)place, dst);
      }
      std::swap(src, dst);
    }
  }
  SMESH_HIP(hipGetLastError());
  uint32_t h_chunks = 0, h_partials = 0;
  SMESH_HIP(hipMemcpyAsync(&h_chunks, m->chunk_start + S, 4, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipMemcpyAsync(&h_partials, m->partial_start + S, 4, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  m->chunks = h_chunks;
  m->partials = h_partials;
  return SMESH_OK;
}

// The member table of `t`, built on first use.  Context locked, device current.
int ensure_members(const SegmentTables& t) {
  if (t.members->built) return SMESH_OK;
  const int status = build_members(t);
  if (status != SMESH_OK) {
    (void)hipStreamSynchronize(t.ctx->stream);
    release_members(t.members);
    return status;
  }
  t.members->built = true;
  return SMESH_OK;
}

// ---- the sums -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float v_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 v_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float v_scale(float w, float v) { return w * v; }
__device__ __forceinline__ float4 v_scale(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }

struct PoolTables {
  const uint32_t *members, *offsets, *chunk_start, *partial_start;
  uint32_t S;
  uint64_t chunks;
};

// One group of 1 << lg lanes owns one chunk; its lanes run over the row's pieces.  T = float4: a piece is 16 bytes (C a multiple
// of four, every array aligned), `per_row` = C / 4; T = float: a piece is one class.  A segment with one chunk writes its pooled
// row; the chunks of every other segment write their partial rows, which k_ss_segment_sums adds up.
// TRIP COUNTS: the search runs 32 steps; the piece loop ceil(per_row / G) turns; the member loop at most kChunk / kInFlight turns,
// its bounds read from tables that were complete before the launch.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ss_chunk_sums(const T* __restrict__ rows, const float* __restrict__ w, PoolTables t, uint32_t per_row,
                                                          int lg, T* __restrict__ pooled, T* __restrict__ partials) {
  const uint64_t j = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> lg;
  const uint32_t G = 1u << lg, gl = threadIdx.x & (G - 1);
  if (j >= t.chunks) return;
  // the chunk's segment: the last s with chunk_start[s] <= j (every segment has at least one chunk, so chunk_start rises strictly)
  uint32_t lo = 0, hi = t.S;
  for (int step = 0; step < 32; step++) {
    if (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (t.chunk_start[mid] <= j) lo = mid;
      else hi = mid;
    }
  }
  const uint32_t s = lo, first = t.chunk_start[s], k = (uint32_t)j - first;
  const uint32_t begin = t.offsets[s] + k * kChunk, end = min(t.offsets[s + 1], begin + kChunk);
  T* const out = t.chunk_start[s + 1] - first == 1 ? pooled + (uint64_t)s * per_row : partials + (uint64_t)(t.partial_start[s] + k) * per_row;
  for (uint32_t p = gl; p < per_row; p += G) {
    T acc = T{};      // +0.0f
    for (uint32_t r = begin; r < end; r += kInFlight) {
      T v[kInFlight];
      float wf[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; u++) {      // one full row per step, all of them issued before the first add
        if (r + u < end) {
          const uint32_t f = t.members[r + u];
          v[u] = rows[(uint64_t)f * per_row + p];
          if (w) wf[u] = w[f];
        }
      }
#pragma unroll
      for (int u = 0; u < kInFlight; u++)        // ascending rank
        if (r + u < end) acc = v_add(acc, w ? v_scale(wf[u], v[u]) : v[u]);
    }
    out[p] = acc;
  }
}

// One group owns one segment and adds the partial rows of its chunks in ascending order; a segment with one chunk has its row already.
// TRIP COUNTS: the piece loop ceil(per_row / G) turns; the partials loop ceil(chunks of s / kInFlight) turns, from chunk_start.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ss_segment_sums(const T* __restrict__ partials, PoolTables t, uint32_t per_row, int lg,
                                                            T* __restrict__ pooled) {
  const uint64_t s = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> lg;
  const uint32_t G = 1u << lg, gl = threadIdx.x & (G - 1);
  if (s >= t.S) return;
  const uint32_t n = t.chunk_start[s + 1] - t.chunk_start[s];
  if (n <= 1) return;
  const T* const mine = partials + (uint64_t)t.partial_start[s] * per_row;
  for (uint32_t p = gl; p < per_row; p += G) {
    T acc = T{};
    for (uint32_t j = 0; j < n; j += kInFlight) {
      T v[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; u++)
        if (j + u < n) v[u] = mine[(uint64_t)(j + u) * per_row + p];
#pragma unroll
      for (int u = 0; u < kInFlight; u++)
        if (j + u < n) acc = v_add(acc, v[u]);
    }
    pooled[s * per_row + p] = acc;
  }
}

// The face form: a plain gather, one lane per piece of the [F, C] output.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ss_gather_faces(const T* __restrict__ rows, const int32_t* __restrict__ ids, const T* __restrict__ pooled,
                                                            uint64_t n, uint32_t per_row, T* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t f = i / per_row;
  const int32_t s = ids[f];
  out[i] = s >= 0 ? pooled[(uint64_t)s * per_row + (i - f * per_row)] : rows[i];
}

int group_bits(uint32_t per_row) {      // the narrowest power of two that covers the row, a wave at the most
  int lg = 0;
  while (lg < 6 && (1u << lg) < per_row) lg++;
  return lg;
}

template <typename T>
void launch_pool(const T* rows, const float* w, const PoolTables& t, uint64_t n_partials, uint32_t per_row, T* pooled, T* partials,
                 hipStream_t st) {
  const int lg = group_bits(per_row);
  if (t.chunks) hipLaunchKernelGGL(k_ss_chunk_sums<T>, grid_for(t.chunks << lg), dim3(kBlock), 0, st, rows, w, t, per_row, lg, pooled, partials);
  if (n_partials) hipLaunchKernelGGL(k_ss_segment_sums<T>, grid_for((uint64_t)t.S << lg), dim3(kBlock), 0, st, (const T*)partials, t, per_row, lg, pooled);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

struct PoolCall {
  const float* weights;
  int weights_memkind, mode;
  float dont_care;
  float* out_rows;
  int32_t* out_labels;
  int out_memkind;
  bool faces;      // the face form
};

int check_pool_call(const PoolCall& p) {
  SMESH_TRY(check_gather_args("segment pool", 1, p.mode, p.out_rows, p.out_labels, p.weights ? p.weights_memkind : SMESH_MEM_HOST, p.out_memkind));
  return SMESH_OK;
}

// Pooled rows of rows that are on the device already.  Context locked, device current.
int pool_device_rows(const SegmentTables& t, DeviceCtx* ctx, const float* d_rows, uint32_t C, const PoolCall& p) {
  hipStream_t st = ctx->stream;
  const uint64_t F = t.F, S = t.S;
  // (S <= F < 2^31 and at most F / 256 + S chunks: a wave per chunk or per segment always fits a launch; one lane per element may not)
  if (div_up(F * C, kBlock) > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "segment pool: F * C must stay below 2^39");
  SMESH_TRY(ensure_members(t));
  const SegmentMembers& m = *t.members;
  TempBlocks tmp;
  const float* d_w = nullptr;
  float *pooled = nullptr, *partials = nullptr, *x = nullptr;
  SMESH_TRY(on_device(ctx, tmp, p.weights, p.weights ? F * 4 : 0, p.weights_memkind, &d_w));
  if (F == 0) d_w = nullptr;
  SMESH_TRY(tmp.alloc(&pooled, S * C * 4));
  SMESH_TRY(tmp.alloc(&partials, m.partials * C * 4));
  if (p.faces) SMESH_TRY(tmp.alloc(&x, F * C * 4));
  const PoolTables pt = {m.members, m.offsets, m.chunk_start, m.partial_start, (uint32_t)S, m.chunks};
  const bool wide = C % 4 == 0 && aligned16(d_rows) && aligned16(pooled) && aligned16(partials) && aligned16(x);
  if (wide) launch_pool(reinterpret_cast<const float4*>(d_rows), d_w, pt, m.partials, C / 4, reinterpret_cast<float4*>(pooled), reinterpret_cast<float4*>(partials), st);
  else launch_pool(d_rows, d_w, pt, m.partials, C, pooled, partials, st);
  if (p.faces && F) {
    if (wide)
      hipLaunchKernelGGL(k_ss_gather_faces<float4>, grid_for(F * C / 4), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(d_rows), t.ids,
                         reinterpret_cast<const float4*>(pooled), F * C / 4, C / 4, reinterpret_cast<float4*>(x));
    else
      hipLaunchKernelGGL(k_ss_gather_faces<float>, grid_for(F * C), dim3(kBlock), 0, st, d_rows, t.ids, (const float*)pooled, F * C, C, x);
  }
  SMESH_HIP(hipGetLastError());
  // the finishing step of smesh_vertices.h (vertices.hip); it returns when the outputs are complete
  return p.faces ? smesh_rows_finish(ctx, x, F, C, p.mode, p.dont_care, p.out_rows, p.out_labels, p.out_memkind)
                 : smesh_rows_finish(ctx, pooled, S, C, p.mode, p.dont_care, p.out_rows, p.out_labels, p.out_memkind);
}

int pool_rows(smesh_face_segments_t* sg, const float* rows, int rows_memkind, uint32_t C, const PoolCall& p) {
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(sg, &t));
  SMESH_TRY(check_pool_call(p));
  if (C == 0) return fail(SMESH_ERR_INVALID, "segment pool: the class count must be positive");
  if (!memkind_ok(rows_memkind)) return fail(SMESH_ERR_INVALID, "segment pool: bad memory kind");
  if (t.F && !rows) return fail(SMESH_ERR_INVALID, "segment pool: NULL rows");
  std::lock_guard<std::recursive_mutex> lock(t.ctx->mu);
  SMESH_HIP(hipSetDevice(t.ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(t.ctx, tmp, rows, (size_t)t.F * C * 4, rows_memkind, &d_rows));
  return pool_device_rows(t, t.ctx, d_rows, C, p);
}

int pool_aggregator(smesh_aggregator_t* ag, smesh_face_segments_t* sg, const PoolCall& p) {
  if (!ag) return fail(SMESH_ERR_INVALID, "NULL argument");
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(sg, &t));
  SMESH_TRY(check_pool_call(p));
  return smesh_aggregator_with_final_rows(ag, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("segment pool", "segments", ctx, t.ctx, P, t.F));
    return pool_device_rows(t, ctx, d_rows, C, p);
  });
}

// ---- face areas -----------------------------------------------------------------------------------------------------------------
// The normal and its length as k_fg_normals (face_graph.hip) computes them; half the length is the area.
__global__ __launch_bounds__(kBlock) void k_ss_face_areas(const int32_t* __restrict__ faces, uint64_t F, uint64_t V, const float* __restrict__ vertices,
                                                          float* __restrict__ area, uint32_t* __restrict__ bad) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || (uint64_t)i0 >= V || (uint64_t)i1 >= V || (uint64_t)i2 >= V) {
    atomicOr(bad, 1u);
    area[f] = 0.0f;
    return;
  }
  const float* const p0 = vertices + (uint64_t)i0 * 3;
  const float* const p1 = vertices + (uint64_t)i1 * 3;
  const float* const p2 = vertices + (uint64_t)i2 * 3;
  const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  area[f] = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
}

// ---- the despeckle by a measure: plain gathers --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ss_despeckle_labels(const int32_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                                const float* __restrict__ measure, float minimum, uint64_t F,
                                                                int32_t* __restrict__ out, unsigned long long* __restrict__ removed) {
  uint32_t mine = 0;
  for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < F; f += (uint64_t)gridDim.x * kBlock) {      // strides over F items
    const int32_t lf = labels[f];
    const bool kept = lf >= 0 && measure[ids[f]] >= minimum;      // (false for a NaN on either side)
    mine += lf >= 0 && !kept ? 1u : 0u;
    out[f] = kept ? lf : -1;
  }
  block_count_add(mine, removed);
}

__global__ __launch_bounds__(kBlock) void k_ss_failing(const float* __restrict__ measure, float minimum, uint64_t S,
                                                       unsigned long long* __restrict__ removed) {
  uint32_t mine = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kBlock) mine += measure[s] >= minimum ? 0u : 1u;
  block_count_add(mine, removed);
}

// T = float4: one lane per 16 bytes (C a multiple of four, both arrays aligned), `per_row` = C / 4; T = float: one lane per element.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ss_despeckle_rows(const T* __restrict__ rows, const int32_t* __restrict__ ids,
                                                              const float* __restrict__ measure, float minimum, uint64_t n, uint32_t per_row,
                                                              T* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T v = rows[i];
  const int32_t s = ids[i / per_row];
  if (s >= 0 && !(measure[s] >= minimum)) v = T{};      // +0.0f in every class
  out[i] = v;
}

int check_measure(const SegmentTables& t, const float* measure, int measure_memkind) {
  if (!memkind_ok(measure_memkind)) return fail(SMESH_ERR_INVALID, "segment despeckle: bad memory kind");
  if (t.S && !measure) return fail(SMESH_ERR_INVALID, "segment despeckle: NULL measure");
  return SMESH_OK;
}

// The rows form over rows that are on the device already.  Context locked, device current.
int despeckle_device_rows(const SegmentTables& t, DeviceCtx* ctx, const float* measure, int measure_memkind, float minimum, const float* d_rows,
                          uint32_t C, float* out_rows, int out_memkind) {
  hipStream_t st = ctx->stream;
  const uint64_t elems = t.F * C;
  if (elems == 0) return SMESH_OK;
  if (div_up(elems, kBlock) > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "segment despeckle: F * C must stay below 2^39");
  TempBlocks tmp;
  const float* d_measure = nullptr;
  Out<float> out;
  SMESH_TRY(on_device(ctx, tmp, measure, t.S * 4, measure_memkind, &d_measure));
  SMESH_TRY(out.init(tmp, out_rows, elems * 4, out_memkind));
  float* const d_out = out.dev;
  if (C % 4 == 0 && aligned16(d_rows) && aligned16(d_out))
    hipLaunchKernelGGL(k_ss_despeckle_rows<float4>, grid_for(elems / 4), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(d_rows), t.ids,
                       d_measure, minimum, elems / 4, C / 4, reinterpret_cast<float4*>(d_out));
  else
    hipLaunchKernelGGL(k_ss_despeckle_rows<float>, grid_for(elems), dim3(kBlock), 0, st, d_rows, t.ids, d_measure, minimum, elems, C, d_out);
  SMESH_HIP(hipGetLastError());
  SMESH_TRY(out.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

}  // namespace

extern "C" {

int smesh_segment_stats_face_areas(const smesh_face_graph_t* graph, const int32_t* faces, const float* vertices, int vertices_memkind,
                                   float* out_areas, int out_memkind) {
  DeviceCtx* ctx = nullptr;
  const uint32_t *offsets = nullptr, *nbr = nullptr;
  uint64_t F = 0, nnz = 0, V = 0;
  SMESH_TRY(smesh_face_graph_tables(graph, &ctx, &offsets, &nbr, &F, &nnz));
  SMESH_TRY(smesh_face_graph_size(graph, nullptr, &V, nullptr));
  if (!memkind_ok(vertices_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "face areas: bad memory kind");
  if (F && (!faces || !vertices || !out_areas)) return fail(SMESH_ERR_INVALID, "face areas: NULL argument");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  if (F == 0) return SMESH_OK;
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  const int32_t* d_faces = nullptr;
  const float* d_vertices = nullptr;
  uint32_t* bad = nullptr;
  Out<float> out;
  SMESH_TRY(on_device(ctx, tmp, faces, F * 12, SMESH_MEM_HOST, &d_faces));
  SMESH_TRY(on_device(ctx, tmp, vertices, V * 12, vertices_memkind, &d_vertices));
  SMESH_TRY(tmp.alloc(&bad, 16));
  SMESH_TRY(out.init(tmp, out_areas, F * 4, out_memkind));
  SMESH_HIP(hipMemsetAsync(bad, 0, 16, st));
  hipLaunchKernelGGL(k_ss_face_areas, grid_for(F), dim3(kBlock), 0, st, d_faces, F, V, d_vertices, out.dev, bad);
  SMESH_HIP(hipGetLastError());
  uint32_t h_bad = 0;
  SMESH_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
  SMESH_TRY(out.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (h_bad) return fail(SMESH_ERR_INVALID, "face areas: a face index lies outside [0, " + std::to_string(V) + ")");
  return SMESH_OK;
}

int smesh_segment_stats_members(smesh_face_segments_t* sg, uint32_t* offsets, uint32_t* members, int out_memkind) {
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(sg, &t));
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "segment members: bad memory kind");
  std::lock_guard<std::recursive_mutex> lock(t.ctx->mu);
  SMESH_HIP(hipSetDevice(t.ctx->device));
  SMESH_TRY(ensure_members(t));
  SMESH_TRY(copy_out<uint32_t>(offsets, t.members->offsets, (t.S + 1) * 4, out_memkind, t.ctx->stream));
  SMESH_TRY(copy_out<uint32_t>(members, t.members->members, t.labelled * 4, out_memkind, t.ctx->stream));
  SMESH_HIP(hipStreamSynchronize(t.ctx->stream));
  return SMESH_OK;
}

int smesh_segment_stats_pool(smesh_face_segments_t* sg, const float* rows, int rows_memkind, uint32_t C, const float* face_weights,
                             int weights_memkind, int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  return pool_rows(sg, rows, rows_memkind, C, {face_weights, weights_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind, false});
}

int smesh_segment_stats_pool_faces(smesh_face_segments_t* sg, const float* rows, int rows_memkind, uint32_t C, const float* face_weights,
                                   int weights_memkind, int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels,
                                   int out_memkind) {
  return pool_rows(sg, rows, rows_memkind, C, {face_weights, weights_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind, true});
}

int smesh_aggregator_segment_stats_pool(smesh_aggregator_t* ag, smesh_face_segments_t* sg, const float* face_weights, int weights_memkind,
                                        int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  return pool_aggregator(ag, sg, {face_weights, weights_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind, false});
}

int smesh_aggregator_segment_stats_pool_faces(smesh_aggregator_t* ag, smesh_face_segments_t* sg, const float* face_weights, int weights_memkind,
                                              int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  return pool_aggregator(ag, sg, {face_weights, weights_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind, true});
}

int smesh_segment_stats_despeckle_labels(const smesh_face_segments_t* sg, const float* measure, int measure_memkind, float minimum,
                                         int32_t* out_labels, int out_memkind, uint64_t* removed_faces, uint64_t* removed_segments) {
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(const_cast<smesh_face_segments_t*>(sg), &t));
  SMESH_TRY(check_measure(t, measure, measure_memkind));
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "segment despeckle: bad memory kind");
  if (t.F && !out_labels) return fail(SMESH_ERR_INVALID, "segment despeckle: NULL out_labels");
  DeviceCtx* ctx = t.ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  if (removed_faces) *removed_faces = 0;
  if (removed_segments) *removed_segments = 0;
  if (t.F == 0) return SMESH_OK;
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  const float* d_measure = nullptr;
  Out<int32_t> out;
  unsigned long long* removed = nullptr;      // [0] faces, [1] segments
  SMESH_TRY(on_device(ctx, tmp, measure, t.S * 4, measure_memkind, &d_measure));
  SMESH_TRY(out.init(tmp, out_labels, t.F * 4, out_memkind));
  SMESH_TRY(tmp.alloc(&removed, 16));
  SMESH_HIP(hipMemsetAsync(removed, 0, 16, st));
  hipLaunchKernelGGL(k_ss_despeckle_labels, count_grid(t.F), dim3(kBlock), 0, st, t.labels, t.ids, d_measure, minimum, t.F, out.dev, removed);
  if (removed_segments && t.S) hipLaunchKernelGGL(k_ss_failing, count_grid(t.S), dim3(kBlock), 0, st, d_measure, minimum, t.S, removed + 1);
  SMESH_HIP(hipGetLastError());
  unsigned long long h_removed[2] = {0, 0};
  SMESH_HIP(hipMemcpyAsync(h_removed, removed, 16, hipMemcpyDeviceToHost, st));
  SMESH_TRY(out.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (removed_faces) *removed_faces = h_removed[0];
  if (removed_segments) *removed_segments = h_removed[1];
  return SMESH_OK;
}

int smesh_segment_stats_despeckle_rows(const smesh_face_segments_t* sg, const float* measure, int measure_memkind, float minimum,
                                       const float* rows, int rows_memkind, uint32_t C, float* out_rows, int out_memkind) {
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(const_cast<smesh_face_segments_t*>(sg), &t));
  SMESH_TRY(check_measure(t, measure, measure_memkind));
  if (C == 0) return fail(SMESH_ERR_INVALID, "segment despeckle: the class count must be positive");
  if (!memkind_ok(rows_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "segment despeckle: bad memory kind");
  if (t.F && (!rows || !out_rows)) return fail(SMESH_ERR_INVALID, "segment despeckle: NULL rows");
  std::lock_guard<std::recursive_mutex> lock(t.ctx->mu);
  SMESH_HIP(hipSetDevice(t.ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(t.ctx, tmp, rows, (size_t)t.F * C * 4, rows_memkind, &d_rows));
  return despeckle_device_rows(t, t.ctx, measure, measure_memkind, minimum, d_rows, C, out_rows, out_memkind);
}

int smesh_aggregator_segment_stats_despeckle(smesh_aggregator_t* ag, const smesh_face_segments_t* sg, const float* measure, int measure_memkind,
                                             float minimum, float* out_rows, int out_memkind) {
  if (!ag) return fail(SMESH_ERR_INVALID, "NULL argument");
  SegmentTables t;
  SMESH_TRY(smesh_face_segments_tables(const_cast<smesh_face_segments_t*>(sg), &t));
  SMESH_TRY(check_measure(t, measure, measure_memkind));
  if (!memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "segment despeckle: bad memory kind");
  if (t.F && !out_rows) return fail(SMESH_ERR_INVALID, "segment despeckle: NULL out_rows");
  return smesh_aggregator_with_final_rows(ag, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("segment despeckle", "segments", ctx, t.ctx, P, t.F));
    return despeckle_device_rows(t, ctx, measure, measure_memkind, minimum, d_rows, C, out_rows, out_memkind);
  });
}

}  // extern "C"
