// depth_weights.hip -- fusion gated by sensor depth (include/smesh_depth.h, where the rule is stated to the bit): k_depth_weights, its
// launcher, smesh_depth_weights and smesh_fuse_views_depth.  The views of a gated call are rasterised and fused by raster.hip's
// smesh_renderer_fuse_views_gated, which calls back here once per group of up to eight views for their weights planes.
//
// Per output pixel (X, Y) of view v:  sx = ((2X + 1) w) div (2W),  sy = ((2Y + 1) h) div (2H)   (src_index, nearest_rule.hpp)
//                                     raw = sensor_v[sx * s0 + sy * s1];   d_s = float(raw) * scale
//                                     t = abs_tol + rel_tol * d_s;   diff = |depth_v[X * H + Y] - d_s|
//                                     out_v[X * H + Y] = background / far / missing / inconsistent ? 0 (missing, kept: w_in) : w_in
// Single float32 operations, never fused (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "depth_gate.hpp"
#include "nearest_rule.hpp"
#include "../../include/smesh_depth.h"
#include "../../include/smesh_half.h"

#include <atomic>
#include <cmath>
#include <mutex>

#pragma clang fp contract(off)

using namespace smesh;

// fusion.hip
uint32_t smesh_aggregator_classes(smesh_aggregator* a);

namespace {

constexpr uint32_t kChunk = 4096;   // output pixels per workgroup: 256 lanes x 4 rounds x 4 pixels
constexpr int kCounts = 4;          // visible, far, missing, inconsistent
constexpr uint32_t kXcds = 8;       // accelerator dies of the MI355X: consecutive workgroups of a launch go to them in turn

std::atomic<uint64_t> g_launches{0};

struct GateView {
  const float* depth;
  const float* w_in;        // or null
  float* w_out;
  const void* sensor;
  uint32_t W, H;
  uint32_t vec;             // the three planes are 16-byte aligned: four pixels per load and store
};

struct GateArgs {
  GateView v[kGroup];
  int64_t s0, s1;           // element strides of the sensor images
  uint32_t w, h;
  float scale, abs_tol, rel_tol, max_depth;
  uint32_t missing_keep;
  unsigned long long* counts;   // [views][kCounts], or null
};

__device__ __forceinline__ bool sample_missing(uint16_t raw) { return raw == 0; }
__device__ __forceinline__ bool sample_missing(float raw) { return !(raw > 0.0f) || !isfinite(raw); }

// The rule for one pixel: its weight, and in `flags` bit 0 visible, bit 1 far, bit 2 missing, bit 3 inconsistent.
template <typename T>
__device__ __forceinline__ float gate_pixel(const GateArgs& a, const GateView& g, const T* __restrict__ sensor, uint32_t X, uint32_t Y, float d_r,
                                            float w_in, uint32_t& flags) {
  flags = 0u;
  if (!isfinite(d_r)) return 0.0f;                        // background (a NaN depth cannot be compared with anything either)
  flags = 1u;
  if (d_r > a.max_depth) { flags |= 2u; return 0.0f; }
  const uint64_t sx = src_index(X, a.w, g.W), sy = src_index(Y, a.h, g.H);
  const T raw = sensor[sx * (uint64_t)a.s0 + sy * (uint64_t)a.s1];
  if (sample_missing(raw)) { flags |= 4u; return a.missing_keep ? w_in : 0.0f; }
  const float d_s = (float)raw * a.scale;
  const float t = a.abs_tol + a.rel_tol * d_s;
  const float diff = fabsf(d_r - d_s);
  if (!(diff <= t)) { flags |= 8u; return 0.0f; }
  return w_in;
}

// One lane per output pixel, lanes along the output's y; blockIdx.y is the view, a workgroup takes kChunk consecutive pixels of it
// (a view smaller than the launch's largest, and the rounding of the grid to the XCDs, leave workgroups idle).  A lane takes four consecutive pixels per round: one
// 16-byte load of the depth plane (and of w_in), one 16-byte store -- or, in an unaligned plane and for the last N mod 4 pixels, the
// same pixels one by one.  Every lane of a wave reaches every ballot: the loop bounds are uniform, out-of-range pixels carry no flags.
template <typename T>
__global__ __launch_bounds__(256) void k_depth_weights(GateArgs a) {
  const GateView& g = a.v[blockIdx.y];
  const uint32_t N = g.W * g.H;   // (< 2^29)
  // Workgroups go to the eight XCDs in turn (gridDim.x is a multiple of eight): XCD j takes the j-th run of consecutive chunks, so the
  // lines of a transposed source, which neighbouring output columns share, are fetched into one L2 and not into all eight.
  const uint32_t per_xcd = gridDim.x / kXcds;
  const uint32_t base = ((blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds) * kChunk;
  if (base >= N) return;          // (uniform over the workgroup)
  const T* __restrict__ sensor = static_cast<const T*>(g.sensor);
  uint32_t cnt[kCounts] = {0u, 0u, 0u, 0u};   // per wave: every lane holds the same values
  for (uint32_t round = 0; round < kChunk / 1024u; round++) {
    const uint32_t i0 = base + round * 1024u + threadIdx.x * 4u;
    uint32_t X = 0u, Y = 0u;
    if (i0 < N) { X = i0 / g.H; Y = i0 - X * g.H; }
    float d[4] = {0.f, 0.f, 0.f, 0.f}, wi[4] = {1.f, 1.f, 1.f, 1.f}, wo[4];
    uint32_t fl[4] = {0u, 0u, 0u, 0u};
    const bool whole = g.vec && i0 + 3u < N;
    if (whole) {
      const float4 q = *reinterpret_cast<const float4*>(g.depth + i0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
      if (g.w_in) {
        const float4 p = *reinterpret_cast<const float4*>(g.w_in + i0);
        wi[0] = p.x; wi[1] = p.y; wi[2] = p.z; wi[3] = p.w;
      }
    } else {
      for (uint32_t e = 0; e < 4u; e++)
        if (i0 + e < N) {
          d[e] = g.depth[i0 + e];
          if (g.w_in) wi[e] = g.w_in[i0 + e];
        }
    }
    for (uint32_t e = 0; e < 4u; e++) {
      wo[e] = 0.0f;
      if (i0 + e < N) wo[e] = gate_pixel<T>(a, g, sensor, X, Y, d[e], wi[e], fl[e]);
      if (++Y == g.H) { Y = 0u; X++; }
    }
    if (whole) {
      *reinterpret_cast<float4*>(g.w_out + i0) = make_float4(wo[0], wo[1], wo[2], wo[3]);
    } else {
      for (uint32_t e = 0; e < 4u; e++)
        if (i0 + e < N) g.w_out[i0 + e] = wo[e];
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

// What every entry point of smesh_depth.h refuses about the sensor images and the gate.
int depth_check(int dt, const int64_t* strides, int mem, uint64_t w, uint64_t h, const smesh_depth_gate_t* gate) {
  if (!gate) return fail(SMESH_ERR_INVALID, "NULL depth gate");
  if (dt != SMESH_DEPTH_U16 && dt != SMESH_DEPTH_F32) return fail(SMESH_ERR_INVALID, "bad sensor depth dtype");
  if (mem != SMESH_MEM_HOST && mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (strides && (strides[0] < 0 || strides[1] < 0)) return fail(SMESH_ERR_INVALID, "sensor depth: negative strides are not supported");
  if (w == 0 || h == 0) return fail(SMESH_ERR_INVALID, "an empty sensor depth image cannot be sampled");
  if (w > 65536 || h > 65536) return fail(SMESH_ERR_INVALID, "sensor depth image too large: at most 65536 pixels a side");
  if (std::isnan(gate->scale) || gate->scale < 0.0f) return fail(SMESH_ERR_INVALID, "depth gate: scale must be a number >= 0");
  if (std::isnan(gate->abs_tol) || gate->abs_tol < 0.0f) return fail(SMESH_ERR_INVALID, "depth gate: abs_tol must be a number >= 0");
  if (std::isnan(gate->rel_tol) || gate->rel_tol < 0.0f) return fail(SMESH_ERR_INVALID, "depth gate: rel_tol must be a number >= 0");
  if (std::isnan(gate->max_depth)) return fail(SMESH_ERR_INVALID, "depth gate: max_depth must be a number (+inf: none)");
  return SMESH_OK;
}

struct SensorDesc {
  int dtype;
  int64_t s0, s1;
  uint64_t w, h;
  size_t bytes() const { return (size_t)(1 + (w - 1) * (uint64_t)s0 + (h - 1) * (uint64_t)s1) * (dtype == SMESH_DEPTH_U16 ? 2u : 4u); }
};

SensorDesc sensor_desc(int dt, const int64_t* strides, uint64_t w, uint64_t h) {
  return SensorDesc{dt, strides ? strides[0] : (int64_t)h, strides ? strides[1] : 1, w, h};
}

// k_depth_weights for m <= kGroup views on the context's main stream: `sensors[v]` in device memory, `counts_dev` [m][kCounts]
// zeroed by the caller, or null.  The caller has checked the arguments and holds the context's lock.
int launch(DeviceCtx* ctx, const GatedView* views, const void* const* sensors, int m, const SensorDesc& sd, const smesh_depth_gate_t& gate,
           unsigned long long* counts_dev) {
  GateArgs a;
  uint64_t maxN = 0;
  for (int v = 0; v < kGroup; v++) {
    const GatedView& s = views[v < m ? v : 0];
    a.v[v] = GateView{s.depth, s.w_in, s.w_out, sensors[v < m ? v : 0], (uint32_t)s.W, (uint32_t)s.H,
                      (aligned16(s.depth) && aligned16(s.w_out) && (!s.w_in || aligned16(s.w_in))) ? 1u : 0u};
    if (v < m) maxN = std::max(maxN, s.W * s.H);
  }
  a.s0 = sd.s0; a.s1 = sd.s1;
  a.w = (uint32_t)sd.w; a.h = (uint32_t)sd.h;
  a.scale = gate.scale; a.abs_tol = gate.abs_tol; a.rel_tol = gate.rel_tol; a.max_depth = gate.max_depth;
  a.missing_keep = gate.missing_keep ? 1u : 0u;
  a.counts = counts_dev;
  if (maxN == 0) return SMESH_OK;
  const dim3 grid(kXcds * (uint32_t)div_up(div_up(maxN, kChunk), kXcds), (uint32_t)m), block(256);
  if (sd.dtype == SMESH_DEPTH_U16) hipLaunchKernelGGL(k_depth_weights<uint16_t>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_depth_weights<float>, grid, block, 0, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  return SMESH_OK;
}

// The weights of a group: host sensor images staged side by side at their own size, one launch, the counts copied out.
int gate_group(DeviceCtx* ctx, DepthScratch& scratch, const GatedView* views, const void* const* sensors, int mem, int m, const SensorDesc& sd,
               const smesh_depth_gate_t& gate, uint64_t* counts_host) {
  const void* dev[kGroup];
  for (int v = 0; v < m; v++) dev[v] = sensors[v];
  if (mem == SMESH_MEM_HOST) {
    const size_t bytes = sd.bytes(), slot = round256(bytes);
    SMESH_TRY(scratch.sensor.reserve(slot * (size_t)m));
    for (int v = 0; v < m; v++) {
      char* d = static_cast<char*>(scratch.sensor.ptr) + slot * (size_t)v;
      SMESH_HIP(hipMemcpyAsync(d, sensors[v], bytes, hipMemcpyHostToDevice, ctx->stream));
      dev[v] = d;
    }
    SMESH_HIP(hipStreamSynchronize(ctx->stream));   // the caller may reuse its host arrays once we return
  }
  unsigned long long* counts_dev = nullptr;
  if (counts_host) {
    SMESH_TRY(scratch.counts.reserve(sizeof(unsigned long long) * kGroup * kCounts));
    counts_dev = static_cast<unsigned long long*>(scratch.counts.ptr);
    SMESH_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * kGroup * kCounts, ctx->stream));
  }
  SMESH_TRY(launch(ctx, views, dev, m, sd, gate, counts_dev));
  if (counts_host) {
    SMESH_HIP(hipMemcpyAsync(counts_host, counts_dev, sizeof(unsigned long long) * (size_t)m * kCounts, hipMemcpyDeviceToHost, ctx->stream));
    SMESH_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SMESH_OK;
}

}  // namespace

// (context.cpp: the read-only option "depth_weights_launches"; view_weights.hip: a depth gate behind the view weights -- depth_gate.hpp)
namespace smesh {
uint64_t smesh_depth_weights_launches() { return g_launches.load(); }

int depth_gate_check(int dtype, const int64_t* strides, int memkind, uint64_t w, uint64_t h, const smesh_depth_gate_t* gate) {
  return depth_check(dtype, strides, memkind, w, h, gate);
}

int depth_gate_group(DeviceCtx* ctx, DepthScratch& scratch, const GatedView* views, const DepthGateCall& call, uint64_t first, int m,
                     uint64_t* counts_host) {
  return gate_group(ctx, scratch, views, call.sensors + first, call.memkind, m, sensor_desc(call.dtype, call.strides, call.w, call.h), call.gate,
                    counts_host);
}

int depth_image_input(smesh_aggregator* aggregator, int image_kind, ViewInput* in) {
  const uint32_t C = smesh_aggregator_classes(aggregator);
  switch (image_kind) {
    case SMESH_DEPTH_IMG_F32: *in = ViewInput::f32(nullptr); break;
    case SMESH_DEPTH_IMG_F16: *in = ViewInput::half(nullptr, SMESH_PROBS_F16); break;
    case SMESH_DEPTH_IMG_BF16: *in = ViewInput::half(nullptr, SMESH_PROBS_BF16); break;
    case SMESH_DEPTH_IMG_LABELS_U8:
      if (C > 255u) return fail(SMESH_ERR_INVALID, "a uint8 label plane holds at most 255 classes");
      *in = ViewInput::labels(nullptr, 1);
      break;
    case SMESH_DEPTH_IMG_LABELS_U16:
      if (C > 65535u) return fail(SMESH_ERR_INVALID, "label images need an aggregator of at most 65535 classes");
      *in = ViewInput::labels(nullptr, 2);
      break;
    default: return fail(SMESH_ERR_INVALID, "bad image kind");
  }
  return SMESH_OK;
}
}  // namespace smesh

extern "C" int smesh_depth_weights(const float* depth, uint64_t W, uint64_t H, const void* sensor, int sensor_dtype, const int64_t sensor_strides[2],
                                   int sensor_memkind, uint64_t w, uint64_t h, const smesh_depth_gate_t* gate, const float* weights_in,
                                   float* weights_out, uint64_t* counts, int device) {
  SMESH_TRY(depth_check(sensor_dtype, sensor_strides, sensor_memkind, w, h, gate));
  if (W > 65536 || H > 65536 || W * H >= (1ull << 29))
    return fail(SMESH_ERR_INVALID, "depth plane too large: at most 65536 pixels a side and fewer than 2^29 pixels");
  if (counts) for (int c = 0; c < kCounts; c++) counts[c] = 0;
  if (W == 0 || H == 0) return SMESH_OK;
  if (!depth || !sensor || !weights_out) return fail(SMESH_ERR_INVALID, "NULL argument");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const SensorDesc sd = sensor_desc(sensor_dtype, sensor_strides, w, h);
  const GatedView view{depth, weights_in, weights_out, W, H};
  DepthScratch scratch;   // (this entry point has no handle to keep it in)
  const int status = gate_group(ctx, scratch, &view, &sensor, sensor_memkind, 1, sd, *gate, counts);
  scratch.release();      // (waits for the device where something was staged)
  return status;
}

extern "C" int smesh_fuse_views_depth(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                      const void* const* images, int image_kind, const float* const* weights, const void* const* sensors,
                                      int sensor_dtype, const int64_t sensor_strides[2], int sensor_memkind, uint64_t w, uint64_t h,
                                      const smesh_depth_gate_t* gate, uint64_t* counts) {
  if (!renderer || !aggregator || (n && (!cameras || !images || !sensors))) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(depth_check(sensor_dtype, sensor_strides, sensor_memkind, w, h, gate));
  ViewInput in;
  SMESH_TRY(depth_image_input(aggregator, image_kind, &in));
  for (uint64_t i = 0; i < n; i++)
    if (!sensors[i]) return fail(SMESH_ERR_INVALID, "NULL sensor depth image");
  if (counts) for (uint64_t i = 0; i < n * kCounts; i++) counts[i] = 0;
  const SensorDesc sd = sensor_desc(sensor_dtype, sensor_strides, w, h);
  const smesh_depth_gate_t g = *gate;
  return smesh_renderer_fuse_views_gated(renderer, aggregator, cameras, n, in, images, weights,
                                         [&](DeviceCtx* ctx, DepthScratch& scratch, uint64_t first, int m, const GatedView* views) -> int {
                                           return gate_group(ctx, scratch, views, sensors + first, sensor_memkind, m, sd, g,
                                                             counts ? counts + first * kCounts : nullptr);
                                         });
}
