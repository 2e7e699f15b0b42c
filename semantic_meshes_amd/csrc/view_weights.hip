// view_weights.hip -- fusion weighted by viewing geometry (include/smesh_view_weights.h, where the rule is stated to the bit):
// k_face_normals, k_view_weights, their launchers, smesh_view_weights and smesh_fuse_views_view_weights.  The views of a weighted call
// are rasterised and fused by raster.hip's smesh_renderer_fuse_views_gated, which calls back here once per group of up to eight views
// for their weights planes; a depth gate given as well runs behind, in place (depth_weights.hip's depth_gate_group).
//
// Per output pixel (X, Y) of view v:  id = idx_v[X * H + Y],  d_r = depth_v[X * H + Y],  n = normals[id]
//                                     a = float(((X + 0.5) - cx) / fx),  b = float(((Y + 0.5) - cy) / fy)        (double, rounded once)
//                                     n_c = R n;  dot = (n_cx*a + n_cy*b) + n_cz;  nn = |n_c|^2;  dd = (a*a + b*b) + 1
//                                     c = |dot| / sqrtf(nn * dd)
//                                     out_v[X * H + Y] = background / far / backfacing / grazing ? 0 : (w_in * c^power) * falloff(d_r)
// Single float32 operations, never fused (-ffp-contract=off); sqrtf and / correctly rounded (no fast-math flag in the Makefile).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "depth_gate.hpp"
#include "../../include/smesh_view_weights.h"

#include <atomic>
#include <cmath>
#include <mutex>

#pragma clang fp contract(off)

using namespace smesh;

namespace {

constexpr uint32_t kChunk = 4096;   // output pixels per workgroup: 256 lanes x 4 rounds x 4 pixels
constexpr int kCounts = 4;          // visible, far, grazing, backfacing
constexpr uint32_t kBackground = 0xFFFFFFFFu;
constexpr uint32_t kXcds = 8;       // accelerator dies of the MI355X: consecutive workgroups of a launch go to them in turn

std::atomic<uint64_t> g_launches{0};

// ---- face normals ------------------------------------------------------------------------------------------------------------------
// One lane per triangle POSITION p of the renderer's face order; the normal goes to the row of the id the index plane holds for it.
__global__ __launch_bounds__(256) void k_face_normals(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                      const uint32_t* __restrict__ prim_id, uint64_t F, uint64_t V, float4* __restrict__ normals) {
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= F) return;
  const uint64_t id = prim_id ? (uint64_t)prim_id[p] : p;
  if (id >= F) return;             // (prim_id is a permutation of [0, F): never taken; the table has F rows)
  const int32_t i0 = faces[3 * p], i1 = faces[3 * p + 1], i2 = faces[3 * p + 2];
  float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i0 >= 0 && i1 >= 0 && i2 >= 0 && (uint64_t)i0 < V && (uint64_t)i1 < V && (uint64_t)i2 < V) {
    const float* v0 = verts + 3 * (uint64_t)i0;
    const float* v1 = verts + 3 * (uint64_t)i1;
    const float* v2 = verts + 3 * (uint64_t)i2;
    const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
    const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
    n.x = e1y * e2z - e1z * e2y;
    n.y = e1z * e2x - e1x * e2z;
    n.z = e1x * e2y - e1y * e2x;
  }
  normals[id] = n;
}

// ---- the weights -------------------------------------------------------------------------------------------------------------------
struct VwView {
  const uint32_t* idx;
  const float* depth;
  const float* w_in;        // or null
  float* w_out;
  double fx, fy, cx, cy;
  float R[9];
  uint32_t W, H;
  uint32_t vec;             // the four planes are 16-byte aligned: four pixels per load and store
};

struct VwArgs {
  VwView v[kGroup];         // 8 x 112 bytes: with the tail below 944 bytes of kernel arguments
  const float4* normals;    // [F]
  unsigned long long* counts;   // [views][kCounts], or null
  uint64_t F;
  uint32_t power, two_sided, falloff;   // falloff: falloff_depth is finite
  float min_cos, max_depth, falloff_depth;
};
static_assert(sizeof(VwArgs) <= 1024, "the cameras of a group travel in the kernel's arguments");

// a or b of the header: the pixel centre through the inverse intrinsics, in double, rounded once
__device__ __forceinline__ float ray_coord(uint32_t p, double c, double f) { return (float)((((double)p + 0.5) - c) / f); }

// The rule for one pixel: its weight, and in `flags` bit 0 visible, bit 1 far, bit 2 grazing, bit 3 backfacing.
__device__ __forceinline__ float view_pixel(const VwArgs& a, const VwView& g, uint32_t id, float d_r, float w_in, float ra, float rb, uint32_t& flags) {
  flags = 0u;
  if (!isfinite(d_r) || id == kBackground || (uint64_t)id >= a.F) return 0.0f;
  flags = 1u;
  if (d_r > a.max_depth) { flags |= 2u; return 0.0f; }
  const float4 n = a.normals[id];
  const float ncx = (g.R[0] * n.x + g.R[1] * n.y) + g.R[2] * n.z;
  const float ncy = (g.R[3] * n.x + g.R[4] * n.y) + g.R[5] * n.z;
  const float ncz = (g.R[6] * n.x + g.R[7] * n.y) + g.R[8] * n.z;
  const float dot = (ncx * ra + ncy * rb) + ncz;
  const float nn = (ncx * ncx + ncy * ncy) + ncz * ncz;
  const float dd = (ra * ra + rb * rb) + 1.0f;
  const float nd = nn * dd;
  float c = 0.0f;
  if (nn > 0.0f && isfinite(nd)) c = fabsf(dot) / sqrtf(nd);
  if (!a.two_sided && dot > 0.0f) { flags |= 8u; return 0.0f; }
  if (!(c >= a.min_cos)) { flags |= 4u; return 0.0f; }
  float gpow = 1.0f;
  for (uint32_t k = 0; k < a.power; k++) gpow = gpow * c;
  float f = 1.0f;
  if (a.falloff) {
    const float q = d_r / a.falloff_depth;
    f = 1.0f / (1.0f + q * q);
  }
  return (w_in * gpow) * f;
}

// One lane per output pixel, lanes along the output's y; blockIdx.y is the view, a workgroup takes kChunk consecutive pixels of it (a
// view smaller than the launch's largest, and the rounding of the grid to the XCDs, leave workgroups idle).  A lane takes four consecutive pixels per round: one 16-byte load of
// the index plane, of the depth plane (and of w_in), one 16-byte store -- or, in an unaligned plane and for the last N mod 4 pixels,
// the same pixels one by one.  The ray's a is computed once per column the four pixels touch.  Every lane of a wave reaches every
// ballot: the loop bounds are uniform, out-of-range pixels carry no flags.
__global__ __launch_bounds__(256) void k_view_weights(VwArgs a) {
  const VwView& g = a.v[blockIdx.y];
  const uint32_t N = g.W * g.H;   // (< 2^29)
  // Workgroups go to the eight XCDs in turn (gridDim.x is a multiple of eight): XCD j takes the j-th run of consecutive chunks, so the
  // rows of the normals table that neighbouring chunks share are fetched into one L2 and not into all eight (measured: DESIGN.md 3.16).
  const uint32_t per_xcd = gridDim.x / kXcds;
  const uint32_t base = ((blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds) * kChunk;
  if (base >= N) return;          // (uniform over the workgroup)
  uint32_t cnt[kCounts] = {0u, 0u, 0u, 0u};   // per wave: every lane holds the same values
  for (uint32_t round = 0; round < kChunk / 1024u; round++) {
    const uint32_t i0 = base + round * 1024u + threadIdx.x * 4u;
    uint32_t X = 0u, Y = 0u;
    if (i0 < N) { X = i0 / g.H; Y = i0 - X * g.H; }
    uint32_t id[4] = {kBackground, kBackground, kBackground, kBackground};
    float d[4] = {0.f, 0.f, 0.f, 0.f}, wi[4] = {1.f, 1.f, 1.f, 1.f}, wo[4];
    uint32_t fl[4] = {0u, 0u, 0u, 0u};
    const bool whole = g.vec && i0 + 3u < N;
    if (whole) {
      const uint4 t = *reinterpret_cast<const uint4*>(g.idx + i0);
      id[0] = t.x; id[1] = t.y; id[2] = t.z; id[3] = t.w;
      const float4 q = *reinterpret_cast<const float4*>(g.depth + i0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
      if (g.w_in) {
        const float4 p = *reinterpret_cast<const float4*>(g.w_in + i0);
        wi[0] = p.x; wi[1] = p.y; wi[2] = p.z; wi[3] = p.w;
      }
    } else {
      for (uint32_t e = 0; e < 4u; e++)
        if (i0 + e < N) {
          id[e] = g.idx[i0 + e];
          d[e] = g.depth[i0 + e];
          if (g.w_in) wi[e] = g.w_in[i0 + e];
        }
    }
    float ra = ray_coord(X, g.cx, g.fx);
    for (uint32_t e = 0; e < 4u; e++) {
      wo[e] = 0.0f;
      if (i0 + e < N) wo[e] = view_pixel(a, g, id[e], d[e], wi[e], ra, ray_coord(Y, g.cy, g.fy), fl[e]);
      if (++Y == g.H) { Y = 0u; X++; ra = ray_coord(X, g.cx, g.fx); }
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

// What every entry point of smesh_view_weights.h refuses about the spec.
int spec_check(const smesh_view_weights_spec_t* s) {
  if (!s) return fail(SMESH_ERR_INVALID, "NULL view weights spec");
  if (s->power < 0 || s->power > SMESH_VW_MAX_POWER) return fail(SMESH_ERR_INVALID, "view weights: power must be in [0, 16]");
  if (std::isnan(s->min_cos) || s->min_cos < 0.0f || s->min_cos > 1.0f) return fail(SMESH_ERR_INVALID, "view weights: min_cos must be in [0, 1]");
  if (std::isnan(s->max_depth)) return fail(SMESH_ERR_INVALID, "view weights: max_depth must be a number (+inf: none)");
  if (std::isnan(s->falloff_depth) || !(s->falloff_depth > 0.0f))
    return fail(SMESH_ERR_INVALID, "view weights: falloff_depth must be a number > 0 (+inf: none)");
  return SMESH_OK;
}

int mesh_check(smesh_renderer* r, RendererMesh* mesh) {
  SMESH_TRY(smesh_renderer_mesh(r, mesh));
  if (mesh->texels)
    return fail(SMESH_ERR_INVALID, "view weights need a triangle renderer: the index plane of a texel renderer holds texel ids, and a texel -> face "
                                   "lookup is not built");
  return SMESH_OK;
}

// The renderer's face-normals table, built on the context's main stream at first use.  The caller holds the renderer's and the
// context's lock.
int ensure_normals(const RendererMesh& mesh, const float4** out) {
  if (!*mesh.normals) {
    float* table = nullptr;
    SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&table), std::max<uint64_t>(mesh.F, 1) * sizeof(float4)));
    if (mesh.F) {
      hipLaunchKernelGGL(k_face_normals, dim3((uint32_t)div_up(mesh.F, 256)), dim3(256), 0, mesh.ctx->stream, mesh.verts, mesh.faces, mesh.prim_id,
                         mesh.F, mesh.V, reinterpret_cast<float4*>(table));
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) { (void)dev_free(table); return fail_hip(e, "k_face_normals", __FILE__, __LINE__); }
    }
    *mesh.normals = table;
  }
  *out = reinterpret_cast<const float4*>(*mesh.normals);
  return SMESH_OK;
}

// k_view_weights for m <= kGroup views on the context's main stream: `views[v]` with its index plane and camera, `counts_dev`
// [m][kCounts] zeroed by the caller, or null.  The caller has checked the arguments and holds the locks.
int launch(DeviceCtx* ctx, const float4* normals, uint64_t F, const GatedView* views, int m, const smesh_view_weights_spec_t& spec,
           unsigned long long* counts_dev) {
  VwArgs a;
  uint64_t maxN = 0;
  for (int v = 0; v < kGroup; v++) {
    const GatedView& s = views[v < m ? v : 0];
    VwView& d = a.v[v];
    d.idx = s.idx; d.depth = s.depth; d.w_in = s.w_in; d.w_out = s.w_out;
    d.fx = s.cam->focal[0]; d.fy = s.cam->focal[1]; d.cx = s.cam->principal[0]; d.cy = s.cam->principal[1];
    for (int k = 0; k < 9; k++) d.R[k] = s.cam->rotation[k];
    d.W = (uint32_t)s.W; d.H = (uint32_t)s.H;
    d.vec = (aligned16(s.idx) && aligned16(s.depth) && aligned16(s.w_out) && (!s.w_in || aligned16(s.w_in))) ? 1u : 0u;
    if (v < m) maxN = std::max(maxN, s.W * s.H);
  }
  a.normals = normals;
  a.counts = counts_dev;
  a.F = F;
  a.power = (uint32_t)spec.power;
  a.two_sided = spec.two_sided ? 1u : 0u;
  a.falloff = std::isinf(spec.falloff_depth) ? 0u : 1u;
  a.min_cos = spec.min_cos; a.max_depth = spec.max_depth; a.falloff_depth = spec.falloff_depth;
  if (maxN == 0) return SMESH_OK;
  const dim3 grid(kXcds * (uint32_t)div_up(div_up(maxN, kChunk), kXcds), (uint32_t)m), block(256);
  hipLaunchKernelGGL(k_view_weights, grid, block, 0, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  return SMESH_OK;
}

// The weights of a group: the normals at first use, one launch, the counts copied out.
int weigh_group(DeviceCtx* ctx, const RendererMesh& mesh, Scratch& counts_scratch, const GatedView* views, int m, const smesh_view_weights_spec_t& spec,
                uint64_t* counts_host) {
  const float4* normals = nullptr;
  SMESH_TRY(ensure_normals(mesh, &normals));
  unsigned long long* counts_dev = nullptr;
  if (counts_host) {
    SMESH_TRY(counts_scratch.reserve(sizeof(unsigned long long) * kGroup * kCounts));
    counts_dev = static_cast<unsigned long long*>(counts_scratch.ptr);
    SMESH_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * kGroup * kCounts, ctx->stream));
  }
  SMESH_TRY(launch(ctx, normals, mesh.F, views, m, spec, counts_dev));
  if (counts_host) {
    SMESH_HIP(hipMemcpyAsync(counts_host, counts_dev, sizeof(unsigned long long) * (size_t)m * kCounts, hipMemcpyDeviceToHost, ctx->stream));
    SMESH_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SMESH_OK;
}

}  // namespace

// (context.cpp: the read-only option "view_weights_launches")
namespace smesh {
uint64_t smesh_view_weights_launches() { return g_launches.load(); }

// (edge_weights.hip: the view weights as the first stage of smesh_fuse_views_weighted -- depth_gate.hpp)
int view_weights_check(smesh_renderer* r, const smesh_view_weights_spec_t* spec, RendererMesh* mesh) {
  SMESH_TRY(spec_check(spec));
  return mesh_check(r, mesh);
}

int view_weights_group(DeviceCtx* ctx, const RendererMesh& mesh, DepthScratch& scratch, const GatedView* views, int m,
                       const smesh_view_weights_spec_t& spec, uint64_t* counts_host) {
  return weigh_group(ctx, mesh, scratch.view_counts, views, m, spec, counts_host);
}
}  // namespace smesh

extern "C" int smesh_view_weights(smesh_renderer_t* renderer, const smesh_camera_t* camera, const uint32_t* indices, const float* depth, uint64_t W,
                                  uint64_t H, const smesh_view_weights_spec_t* spec, const float* weights_in, float* weights_out, uint64_t* counts) {
  if (!renderer || !camera) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(spec_check(spec));
  RendererMesh mesh;
  SMESH_TRY(mesh_check(renderer, &mesh));
  if (W > 65536 || H > 65536 || W * H >= (1ull << 29))
    return fail(SMESH_ERR_INVALID, "index and depth planes too large: at most 65536 pixels a side and fewer than 2^29 pixels");
  if (counts) for (int c = 0; c < kCounts; c++) counts[c] = 0;
  if (W == 0 || H == 0) return SMESH_OK;
  if (W != camera->width || H != camera->height) return fail(SMESH_ERR_INVALID, "the planes must have the camera's resolution");
  if (!indices || !depth || !weights_out) return fail(SMESH_ERR_INVALID, "NULL argument");
  DeviceCtx* ctx = mesh.ctx;
  std::lock_guard<std::mutex> g(*mesh.mu);
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const GatedView view{depth, weights_in, weights_out, W, H, indices, camera};
  Scratch counts_scratch;   // (kept for the call only: the renderer's is its gated driver's)
  const int status = weigh_group(ctx, mesh, counts_scratch, &view, 1, *spec, counts);
  counts_scratch.release();
  return status;
}

extern "C" int smesh_fuse_views_view_weights(smesh_renderer_t* renderer, smesh_aggregator_t* aggregator, const smesh_camera_t* cameras, uint64_t n,
                                             const void* const* images, int image_kind, const float* const* weights,
                                             const smesh_view_weights_spec_t* spec, const void* const* sensors, int sensor_dtype,
                                             const int64_t sensor_strides[2], int sensor_memkind, uint64_t w, uint64_t h, const smesh_depth_gate_t* gate,
                                             uint64_t* view_counts, uint64_t* depth_counts) {
  if (!renderer || !aggregator || (n && (!cameras || !images))) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(spec_check(spec));
  RendererMesh mesh;
  SMESH_TRY(mesh_check(renderer, &mesh));
  if ((sensors != nullptr) != (gate != nullptr)) return fail(SMESH_ERR_INVALID, "sensor depth images and a depth gate go together");
  if (depth_counts && !gate) return fail(SMESH_ERR_INVALID, "depth counts need a depth gate");
  if (gate) {
    SMESH_TRY(depth_gate_check(sensor_dtype, sensor_strides, sensor_memkind, w, h, gate));
    for (uint64_t i = 0; i < n; i++)
      if (!sensors[i]) return fail(SMESH_ERR_INVALID, "NULL sensor depth image");
  }
  ViewInput in;
  SMESH_TRY(depth_image_input(aggregator, image_kind, &in));
  if (view_counts) for (uint64_t i = 0; i < n * kCounts; i++) view_counts[i] = 0;
  if (depth_counts) for (uint64_t i = 0; i < n * kCounts; i++) depth_counts[i] = 0;
  const smesh_view_weights_spec_t s = *spec;
  DepthGateCall call{sensors, sensor_dtype, sensor_memkind, sensor_strides, w, h, gate ? *gate : smesh_depth_gate_t{}};
  return smesh_renderer_fuse_views_gated(
      renderer, aggregator, cameras, n, in, images, weights, [&](DeviceCtx* ctx, DepthScratch& scratch, uint64_t first, int m, const GatedView* views) -> int {
        SMESH_TRY(weigh_group(ctx, mesh, scratch.view_counts, views, m, s, view_counts ? view_counts + first * kCounts : nullptr));
        if (!gate) return SMESH_OK;
        GatedView behind[kGroup];   // the gate reads the planes just written and writes them in place
        for (int v = 0; v < m; v++) { behind[v] = views[v]; behind[v].w_in = views[v].w_out; }
        return depth_gate_group(ctx, scratch, behind, call, first, m, depth_counts ? depth_counts + first * kCounts : nullptr);
      });
}
