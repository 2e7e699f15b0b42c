// edge_weights.hip -- fusion gated at occlusion edges (include/smesh_edge_gate.h, where the rule is stated to the bit): k_edge_weights,
// its launcher, smesh_edge_weights and smesh_fuse_views_weighted.  The views of a weighted call are rasterised and fused by raster.hip's
// smesh_renderer_fuse_views_gated, which calls back here once per group of up to eight views for their weights planes: the view
// weights (view_weights.hip), then the edge gate, then the depth gate (depth_weights.hip), the later stages in place.
//
// Per output pixel (X, Y) of view v:  d = depth_v[X * H + Y];  lo, hi, bg over the window of `radius` around it, inside the image
//                                     t = abs_tol + rel_tol * d
//                                     out_v[X * H + Y] = background / behind / front / silhouette ? 0 : w_in
// Single float32 operations, never fused (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "depth_gate.hpp"
#include "../../include/smesh_edge_gate.h"

#include <atomic>
#include <cmath>
#include <mutex>

#pragma clang fp contract(off)

using namespace smesh;

namespace {

constexpr uint32_t kTX = SMESH_EDGE_TILE_X;       // columns of a tile
constexpr uint32_t kTY = SMESH_EDGE_TILE_Y;       // rows of a tile: one wave's lanes along y
constexpr uint32_t kR = SMESH_EDGE_MAX_RADIUS;
constexpr uint32_t kPitchD = kTY + 2u * kR;       // dwords per column of the depth tile: the tile's first row always sits at kR
constexpr uint32_t kPitchM = kTY;                 // dwords per column of the min / max planes: exactly one 64-bank row (see the x pass)
constexpr uint32_t kPitchB = kTY / 4u;            // dwords per column of the background plane: one bit per row, four rows per dword
constexpr int kCounts = 4;                        // visible, behind, front, silhouette
static_assert(kTY == 64 && kTX % 16 == 0 && kR % 4 == 0, "one wave along a column; sixteen columns per round of the x pass; aligned 16-byte reads");
static_assert(kPitchM % 64 == 0, "the x pass reads the min / max planes in 16 bytes: a pitch of whole bank rows keeps its lane groups apart");

std::atomic<uint64_t> g_launches{0};

// LDS of a workgroup at radius r: (kTX + 2 r) columns of depth, min, max and background words
constexpr size_t lds_bytes(uint32_t r) { return (size_t)(kTX + 2u * r) * (kPitchD + 2u * kPitchM + kPitchB) * 4u; }
static_assert(lds_bytes(kR) <= 64u * 1024u, "LDS per workgroup");

struct EdgeView {
  const float* depth;
  const float* w_in;        // or null
  float* w_out;
  uint32_t W, H;
  uint32_t vec;             // the weights planes are 16-byte aligned and H is a multiple of four: four pixels per load and store
};

struct EdgeArgs {
  EdgeView v[kGroup];
  unsigned long long* counts;   // [views][kCounts], or null
  uint32_t tiles_y;             // tiles along y of the launch's tallest view
  uint32_t radius, behind, front, silhouette;
  float abs_tol, rel_tol;
};

// The rule for one pixel from its window's lo, hi and bg: its weight, and in `flags` bit 0 visible, bit 1 behind, bit 2 front,
// bit 3 silhouette.
__device__ __forceinline__ float edge_pixel(const EdgeArgs& a, float d, float lo, float hi, bool bg, float w_in, uint32_t& flags) {
  flags = 0u;
  if (!(fabsf(d) < INFINITY)) return 0.0f;                // background (NaN, +-inf)
  flags = 1u;
  const float t = a.abs_tol + a.rel_tol * d;
  if (a.behind && (d - lo) > t) { flags |= 2u; return 0.0f; }
  if (a.front && (hi - d) > t) { flags |= 4u; return 0.0f; }
  if (a.silhouette && bg) { flags |= 8u; return 0.0f; }
  return w_in;
}

// blockIdx.y is the view, blockIdx.x a tile of kTX x kTY pixels of it (a view smaller than the launch's largest leaves workgroups
// idle).  Three steps, a barrier between them:
//   load    wave w takes columns w, w + 4, .. of the tile and its halo, a lane one row (and the row 64 further on): coalesced 4-byte
//           loads along y.  Background is stored as NaN, outside the image as +inf: neither wins `<`, neither passes `> hi && < inf`,
//           and only NaN sets bg.
//   y pass  the same waves and columns, lane = row: 2 r + 1 consecutive LDS reads down the column -- 32 consecutive dwords per
//           half-wave, conflict-free at any pitch -- give the column's min, max and background bit over the rows of the window; the
//           bits of four rows are gathered into one dword across lanes.
//   x pass  a lane owns four consecutive rows of one column, sixteen lanes a column, a wave four columns: per window column one
//           16-byte read of the min plane, one of the max plane and one dword of background bits.  A 16-byte LDS read is served in
//           groups of 16 lanes taken from two columns of the wave (lanes 0-3, 12-15 of one and 4-11 of the next, and so on); with a
//           column pitch of whole 64-bank rows the slots a group reads are those of ONE contiguous 256-byte row, so the pass has no
//           bank conflict, which any pitch that is not a multiple of 64 dwords would give it.  weights_in / weights_out move as the
//           same four rows: 16 bytes per lane, or one by one.
// Every lane of a wave reaches every shuffle and ballot: the loop bounds are uniform, pixels outside the image carry no flags.
__global__ __launch_bounds__(256) void k_edge_weights(EdgeArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const EdgeView& g = a.v[blockIdx.y];
  const uint32_t r = a.radius;
  const uint32_t cols = kTX + 2u * r;
  const uint32_t x0 = (blockIdx.x / a.tiles_y) * kTX, y0 = (blockIdx.x % a.tiles_y) * kTY;
  if (x0 >= g.W || y0 >= g.H) return;             // (uniform over the workgroup)
  float* s_d = reinterpret_cast<float*>(lds_raw);
  float* s_lo = s_d + cols * kPitchD;
  float* s_hi = s_lo + cols * kPitchM;
  uint32_t* s_bg = reinterpret_cast<uint32_t*>(s_hi + cols * kPitchM);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const float* __restrict__ depth = g.depth;

  // ---- load: rows y0 - r .. y0 + kTY + r - 1 of columns x0 - r .. x0 + kTX + r - 1, row y0 at index kR of its column
  // (all of a wave's loads are issued before the first is stored: up to 12 columns x 2 rows per lane in flight, one memory latency
  // per tile and not one per column)
  {
    constexpr uint32_t kPerWave = (kTX + 2u * kR) / 4u;
    const uint32_t rows = kTY + 2u * r;
    float v[kPerWave][2];
#pragma unroll
    for (uint32_t i = 0; i < kPerWave; i++) {
      const uint32_t c = wave + 4u * i;
      const int64_t X = (int64_t)x0 + c - r;
      const bool in_x = c < cols && X >= 0 && X < (int64_t)g.W;
#pragma unroll
      for (uint32_t h = 0; h < 2u; h++) {
        const uint32_t j = lane + 64u * h;
        const int64_t Y = (int64_t)y0 + j - r;
        v[i][h] = INFINITY;
        if (in_x && j < rows && Y >= 0 && Y < (int64_t)g.H) v[i][h] = depth[(uint64_t)X * g.H + (uint64_t)Y];
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kPerWave; i++) {
      const uint32_t c = wave + 4u * i;
#pragma unroll
      for (uint32_t h = 0; h < 2u; h++) {
        const uint32_t j = lane + 64u * h;
        // (+inf stays +inf only where it stands for outside the image: a loaded +inf is background like NaN)
        const int64_t X = (int64_t)x0 + c - r, Y = (int64_t)y0 + j - r;
        const bool inside = X >= 0 && X < (int64_t)g.W && Y >= 0 && Y < (int64_t)g.H;
        float w = v[i][h];
        if (inside && !(fabsf(w) < INFINITY)) w = NAN;
        if (c < cols && j < rows) s_d[c * kPitchD + (kR - r) + j] = w;
      }
    }
  }
  __syncthreads();

  // ---- y pass
  for (uint32_t c = wave; c < cols; c += 4u) {
    const float* col = s_d + c * kPitchD + (kR - r) + lane;
    float lo = INFINITY, hi = -INFINITY;
    uint32_t bg = 0u;
    for (uint32_t k = 0; k <= 2u * r; k++) {
      const float v = col[k];
      if (v < lo) lo = v;
      if (v > hi && v < INFINITY) hi = v;
      if (v != v) bg = 1u;
    }
    s_lo[c * kPitchM + lane] = lo;
    s_hi[c * kPitchM + lane] = hi;
    uint32_t m = bg << (lane & 3u);
    m |= (uint32_t)__shfl_xor((int)m, 1);
    m |= (uint32_t)__shfl_xor((int)m, 2);
    if ((lane & 3u) == 0u) s_bg[c * kPitchB + (lane >> 2)] = m;
  }
  __syncthreads();

  // ---- x pass and the rule
  const uint32_t yq = threadIdx.x & 15u;
  uint32_t cnt[kCounts] = {0u, 0u, 0u, 0u};       // per wave: every lane holds the same values
  for (uint32_t x = threadIdx.x >> 4; x < kTX; x += 16u) {
    float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    uint32_t bg = 0u;
    for (uint32_t c = x; c <= x + 2u * r; c++) {
      const float4 l = *reinterpret_cast<const float4*>(s_lo + c * kPitchM + 4u * yq);
      const float4 h = *reinterpret_cast<const float4*>(s_hi + c * kPitchM + 4u * yq);
      bg |= s_bg[c * kPitchB + yq];
      if (l.x < lo[0]) lo[0] = l.x;
      if (l.y < lo[1]) lo[1] = l.y;
      if (l.z < lo[2]) lo[2] = l.z;
      if (l.w < lo[3]) lo[3] = l.w;
      if (h.x > hi[0]) hi[0] = h.x;
      if (h.y > hi[1]) hi[1] = h.y;
      if (h.z > hi[2]) hi[2] = h.z;
      if (h.w > hi[3]) hi[3] = h.w;
    }
    const float4 dq = *reinterpret_cast<const float4*>(s_d + (x + r) * kPitchD + kR + 4u * yq);
    const float d[4] = {dq.x, dq.y, dq.z, dq.w};
    const uint32_t X = x0 + x, Y = y0 + 4u * yq;
    const bool in_x = X < g.W;
    const uint32_t i0 = in_x ? X * g.H + Y : 0u;  // (< 2^29)
    float wi[4] = {1.f, 1.f, 1.f, 1.f}, wo[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t fl[4] = {0u, 0u, 0u, 0u};
    const bool whole = g.vec && in_x && Y + 3u < g.H;
    if (g.w_in) {
      if (whole) {
        const float4 p = *reinterpret_cast<const float4*>(g.w_in + i0);
        wi[0] = p.x; wi[1] = p.y; wi[2] = p.z; wi[3] = p.w;
      } else {
        for (uint32_t e = 0; e < 4u; e++)
          if (in_x && Y + e < g.H) wi[e] = g.w_in[i0 + e];
      }
    }
    for (uint32_t e = 0; e < 4u; e++)
      if (in_x && Y + e < g.H) wo[e] = edge_pixel(a, d[e], lo[e], hi[e], (bg >> e) & 1u, wi[e], fl[e]);
    if (whole) {
      *reinterpret_cast<float4*>(g.w_out + i0) = make_float4(wo[0], wo[1], wo[2], wo[3]);
    } else {
      for (uint32_t e = 0; e < 4u; e++)
        if (in_x && Y + e < g.H) g.w_out[i0 + e] = wo[e];
    }
    if (a.counts) {
      for (uint32_t e = 0; e < 4u; e++)
        for (int c = 0; c < kCounts; c++) cnt[c] += (uint32_t)__popcll(__ballot((fl[e] >> c) & 1u));
    }
  }
  if (a.counts && (threadIdx.x & 63u) == 0u) {
    for (int c = 0; c < kCounts; c++)
      if (cnt[c]) atomicAdd(&a.counts[blockIdx.y * kCounts + c], (unsigned long long)cnt[c]);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What every entry point of smesh_edge_gate.h refuses about the gate.
int edge_check(const smesh_edge_gate_t* g) {
  if (!g) return fail(SMESH_ERR_INVALID, "NULL edge gate");
  if (g->radius < 1 || g->radius > SMESH_EDGE_MAX_RADIUS) return fail(SMESH_ERR_INVALID, "edge gate: radius must be in [1, 8]");
  if (std::isnan(g->abs_tol) || g->abs_tol < 0.0f) return fail(SMESH_ERR_INVALID, "edge gate: abs_tol must be a number >= 0");
  if (std::isnan(g->rel_tol) || g->rel_tol < 0.0f) return fail(SMESH_ERR_INVALID, "edge gate: rel_tol must be a number >= 0");
  if ((g->behind | g->front | g->silhouette) & ~1) return fail(SMESH_ERR_INVALID, "edge gate: behind, front and silhouette must be 0 or 1");
  return SMESH_OK;
}

// k_edge_weights for m <= kGroup views on the context's main stream; `counts_dev` [m][kCounts] zeroed by the caller, or null.  The
// caller has checked the arguments and holds the context's lock.
int launch(DeviceCtx* ctx, const GatedView* views, int m, const smesh_edge_gate_t& gate, unsigned long long* counts_dev) {
  EdgeArgs a;
  uint64_t maxW = 0, maxH = 0;
  for (int v = 0; v < kGroup; v++) {
    const GatedView& s = views[v < m ? v : 0];
    a.v[v] = EdgeView{s.depth, s.w_in, s.w_out, (uint32_t)s.W, (uint32_t)s.H,
                      (aligned16(s.w_out) && (!s.w_in || aligned16(s.w_in)) && s.H % 4 == 0) ? 1u : 0u};
    if (v < m && s.W && s.H) { maxW = std::max(maxW, s.W); maxH = std::max(maxH, s.H); }
  }
  a.counts = counts_dev;
  a.radius = (uint32_t)gate.radius;
  a.behind = (uint32_t)gate.behind; a.front = (uint32_t)gate.front; a.silhouette = (uint32_t)gate.silhouette;
  a.abs_tol = gate.abs_tol; a.rel_tol = gate.rel_tol;
  if (maxW == 0) return SMESH_OK;
  a.tiles_y = (uint32_t)div_up(maxH, kTY);
  const dim3 grid((uint32_t)div_up(maxW, kTX) * a.tiles_y, (uint32_t)m), block(256);
  hipLaunchKernelGGL(k_edge_weights, grid, block, lds_bytes(a.radius), ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  return SMESH_OK;
}

// The weights of a group: one launch, the counts copied out.
int edge_group(DeviceCtx* ctx, Scratch& counts_scratch, const GatedView* views, int m, const smesh_edge_gate_t& gate, uint64_t* counts_host) {
  unsigned long long* counts_dev = nullptr;
  if (counts_host) {
    SMESH_TRY(counts_scratch.reserve(sizeof(unsigned long long) * kGroup * kCounts));
    counts_dev = static_cast<unsigned long long*>(counts_scratch.ptr);
    SMESH_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * kGroup * kCounts, ctx->stream));
  }
  SMESH_TRY(launch(ctx, views, m, gate, counts_dev));
  if (counts_host) {
    SMESH_HIP(hipMemcpyAsync(counts_host, counts_dev, sizeof(unsigned long long) * (size_t)m * kCounts, hipMemcpyDeviceToHost, ctx->stream));
    SMESH_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SMESH_OK;
}

}  // namespace

// (context.cpp: the read-only option "edge_weights_launches")
namespace smesh {
uint64_t smesh_edge_weights_launches() { return g_launches.load(); }
}  // namespace smesh

extern "C" int smesh_edge_weights(const float* depth, uint64_t W, uint64_t H, const smesh_edge_gate_t* gate, const float* weights_in, float* weights_out,
                                  uint64_t* counts, int device) {
  SMESH_TRY(edge_check(gate));
  if (W > 65536 || H > 65536 || W * H >= (1ull << 29))
    return fail(SMESH_ERR_INVALID, "depth plane too large: at most 65536 pixels a side and fewer than 2^29 pixels");
  if (counts) for (int c = 0; c < kCounts; c++) counts[c] = 0;
  if (W == 0 || H == 0) return SMESH_OK;
  if (!depth || !weights_out) return fail(SMESH_ERR_INVALID, "NULL argument");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const GatedView view{depth, weights_in, weights_out, W, H};
  Scratch counts_scratch;   // (this entry point has no handle to keep it in)
  const int status = edge_group(ctx, counts_scratch, &view, 1, *gate, counts);
  counts_scratch.release();
  return status;
}

extern "C" int smesh_fuse_views_weighted(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                         const void* const* images, int image_kind, const float* const* weights,
                                         const smesh_view_weights_spec_t* spec, const smesh_edge_gate_t* edge, const void* const* sensors,
                                         int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind, uint64_t w, uint64_t h,
                                         const smesh_depth_gate_t* gate, uint64_t* view_counts, uint64_t* edge_counts, uint64_t* depth_counts) {
  if (!renderer || !aggregator || (n && (!cameras || !images))) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (!spec && !edge && !sensors && !gate) return fail(SMESH_ERR_INVALID, "a weighted fuse call needs view weights, an edge gate or a depth gate");
  RendererMesh mesh{};
  if (spec) SMESH_TRY(view_weights_check(renderer, spec, &mesh));
  if (edge) SMESH_TRY(edge_check(edge));
  if ((sensors != nullptr) != (gate != nullptr)) return fail(SMESH_ERR_INVALID, "sensor depth images and a depth gate go together");
  if (view_counts && !spec) return fail(SMESH_ERR_INVALID, "view counts need a view weights spec");
  if (edge_counts && !edge) return fail(SMESH_ERR_INVALID, "edge counts need an edge gate");
  if (depth_counts && !gate) return fail(SMESH_ERR_INVALID, "depth counts need a depth gate");
  if (gate) {
    SMESH_TRY(depth_gate_check(sensor_dtype, sensor_strides, sensor_memkind, w, h, gate));
    for (uint64_t i = 0; i < n; i++)
      if (!sensors[i]) return fail(SMESH_ERR_INVALID, "NULL sensor depth image");
  }
  ViewInput in;
  SMESH_TRY(depth_image_input(aggregator, image_kind, &in));
  for (uint64_t* c : {view_counts, edge_counts, depth_counts})
    if (c) for (uint64_t i = 0; i < n * kCounts; i++) c[i] = 0;
  const smesh_view_weights_spec_t s = spec ? *spec : smesh_view_weights_spec_t{};
  const smesh_edge_gate_t e = edge ? *edge : smesh_edge_gate_t{};
  DepthGateCall call{sensors, sensor_dtype, sensor_memkind, sensor_strides, w, h, gate ? *gate : smesh_depth_gate_t{}};
  return smesh_renderer_fuse_views_gated(
      renderer, aggregator, cameras, n, in, images, weights, [&](DeviceCtx* ctx, DepthScratch& scratch, uint64_t first, int m, const GatedView* views) -> int {
        GatedView stage[kGroup];    // a later stage reads the planes the earlier one wrote and writes them in place
        for (int v = 0; v < m; v++) stage[v] = views[v];
        bool written = false;
        auto in_place = [&] { if (!written) { written = true; for (int v = 0; v < m; v++) stage[v].w_in = stage[v].w_out; } };
        if (spec) {
          SMESH_TRY(view_weights_group(ctx, mesh, scratch, stage, m, s, view_counts ? view_counts + first * kCounts : nullptr));
          in_place();
        }
        if (edge) {
          SMESH_TRY(edge_group(ctx, scratch.edge_counts, stage, m, e, edge_counts ? edge_counts + first * kCounts : nullptr));
          in_place();
        }
        if (gate) SMESH_TRY(depth_gate_group(ctx, scratch, stage, call, first, m, depth_counts ? depth_counts + first * kCounts : nullptr));
        return SMESH_OK;
      });
}
