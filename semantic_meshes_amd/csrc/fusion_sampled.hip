// fusion_sampled.hip -- fusion of (w,h,C) class-vector images at the network's resolution into (W,H) views with no camera-resolution
// image anywhere: the kernel, and the entry points of include/smesh_sampled.h.  A translation unit of its own: nothing here is seen by
// k_fuse_tri, k_fuse_tri_h16 or their instance files (fuse_tri.inc.hpp is included for its records and wave helpers only, read-only).
//
// Semantics: what resample-then-fuse gives, to the bit.  For a visible pixel (X,Y) of a view the class vector is
//     p[c] = blend(src[x0,y0,c], src[x1,y0,c], src[x0,y1,c], src[x1,y1,c], fx, fy)          (resize_rule.hpp)
// on the exactly widened source, and -- a 16-bit source -- rounded to the source's dtype and widened again, because the resampled
// image of the other route has the input's dtype.  After that everything is Mesh.h:90-106 as k_fuse_tri_h16 computes it:
//     n  = pixels of p in this view's index image
//     w0 = iew * (1.0f / (float)n) + (1 - iew) * 1.0f
//     w  = w0 * weight[pixel]                       (1.0f without a weights image; the weights image is (W,H))
//     sum = p[0] + p[1] + ... in float32; pixels with !(sum > 0.5f) add nothing
//     Sum: acc[p][c] = acc[p][c] + p[c] * w for every c;  Summax: for c = the first largest class only
// in image order (x major, y fastest), view after view.  Mul, texel renderers, re-ordered meshes, more than kHalfMaxClasses classes,
// a class stride other than 1 and foreign index images get the image resampled by smesh_resize_probs into the aggregator's scratch
// and take the existing entry points unchanged.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "half_scratch.hpp"
#include "resize_rule.hpp"
#include "../../include/smesh_sampled.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>

using namespace smesh;

// fusion.hip
struct smesh_aggregator;
DeviceCtx* smesh_aggregator_ctx(smesh_aggregator* a);
bool smesh_aggregator_can_fuse_triangles(smesh_aggregator* a, uint64_t F);
int smesh_aggregator_refuse_scattered(smesh_aggregator* a, const char* what);
void smesh_aggregator_label_target(smesh_aggregator* a, float** acc, uint64_t* P, uint32_t* C, int* kind, float* iew);
HalfScratch& smesh_aggregator_half_scratch(smesh_aggregator* a);
void smesh_set_last_fuse_instance(int slot, int views);
void smesh_note_fuse_rows_views(DeviceCtx* ctx, const RenderedView* views, int nviews);
// raster.hip
struct smesh_renderer;
DeviceCtx* smesh_renderer_ctx(smesh_renderer* r);
bool smesh_renderer_sampled_native(smesh_renderer* r, smesh_aggregator* a);
int smesh_renderer_fuse_views_sampled(smesh_renderer* r, smesh_aggregator* a, const smesh_camera_t* cams, uint64_t n, const void* const* probs,
                                      const float* const* weights, const ViewInput& in);
int smesh_renderer_add_rendered_input(smesh_aggregator* a, smesh_renderer* r, const uint32_t* idx_dev, const ViewInput& in, const float* weights,
                                      uint64_t W, uint64_t H, int* done);

namespace {

#include "fuse_tri.inc.hpp"
#include "fuse_rows.inc.hpp"

// One view as k_fuse_tri_sampled sees it.  The source image's size, strides and dtype are the call's (SampArgs).
struct SampView {
  const TriFrag* frags;
  const uint32_t* idx;        // index plane [W][H]
  const char* src;            // [w][h][C] of the call's dtype; x and y strides ps0, ps1 in elements, class stride 1
  const float* weights;       // [W][H], may be null
  const uint32_t* big_queue;
  const uint32_t* big_len;    // [0] queue length, [1] "check the masks against the index plane" flag of the render
  double sx, sy;              // (double)w / W and (double)h / H, divided on the host
  uint32_t W, H;
};
template <int NV>
struct SampViews {
  SampView v[NV];
};
struct SampArgs {
  float* acc;                 // [P][C] dense
  uint64_t F;
  uint32_t C;
  float iew;
  uint32_t big_capacity;
  uint32_t tri_blocks;        // blocks 0 .. tri_blocks-1 walk the triangles, the next big_blocks the queues of triangles over 8 x 8 pixels
  uint32_t big_blocks;
  uint32_t dt;                // SMESH_PROBS_* of the source elements (wave-uniform: one branch around the loads, one around the re-rounding)
  uint32_t w, h;              // the source images' size
  uint32_t ps0, ps1;
};

// Eight classes of a row from `p` on, `r` = 1 .. 8 of them inside the row (wave-uniform), widened exactly; the others come out as +0.
// float32: 16-byte pieces of four classes, then 8 and 4 bytes for what is left; 16 bits: 16 bytes, or load_part16's pieces.
// EB: bytes per element; `bf`: the 16-bit elements are bfloat16.
template <int EB>
__device__ __forceinline__ void load_chunk(const char* __restrict__ p, int r, bool bf, float (&v)[8]) {
  if constexpr (EB == 4) {
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(p);
    u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
    if (r == 8) {
      a = *reinterpret_cast<const u32x4_a4*>(q);
      b = *reinterpret_cast<const u32x4_a4*>(q + 4);
    } else {
      u32x2 t2 = {0u, 0u};
      uint32_t t1 = 0u;
      if (r & 4) a = *reinterpret_cast<const u32x4_a4*>(q);
      if (r & 2) t2 = *reinterpret_cast<const u32x2_a4*>(q + (r & 4));
      if (r & 1) t1 = q[r & 6];
      u32x4 rest;   // what follows the 16-byte piece, if there is one
      rest.x = (r & 2) ? t2.x : t1; rest.y = (r & 2) ? t2.y : 0u; rest.z = (r & 2) ? t1 : 0u; rest.w = 0u;
      if (r & 4) b = rest; else a = rest;
    }
    v[0] = __uint_as_float(a.x); v[1] = __uint_as_float(a.y); v[2] = __uint_as_float(a.z); v[3] = __uint_as_float(a.w);
    v[4] = __uint_as_float(b.x); v[5] = __uint_as_float(b.y); v[6] = __uint_as_float(b.z); v[7] = __uint_as_float(b.w);
  } else {
    const uint16_t* __restrict__ q = reinterpret_cast<const uint16_t*>(p);
    u32x4 a = {0u, 0u, 0u, 0u};
    if (r == 8) {
      a = *reinterpret_cast<const u32x4_a2*>(q);
    } else {
      a = load_part16(q, r);
    }
    unpack2(a.x, bf, v[0], v[1]); unpack2(a.y, bf, v[2], v[3]); unpack2(a.z, bf, v[4], v[5]); unpack2(a.w, bf, v[6], v[7]);
  }
}

// The class vector of pixel (X,Y) of view `vw` into CT float32 registers, C <= CT run-time classes with CT = the multiple of eight at
// or above C.  The row is blended in chunks of eight classes -- four corner pieces in, eight blended values out -- so that no instance
// holds four whole corner rows (a 48-slot one would spill).  Any X, Y: the rule clamps its coordinates into the source.
template <int CT, int EB>
__device__ __forceinline__ void sample_row_as(const SampArgs& a, const SampView& vw, uint32_t X, uint32_t Y, bool bf, float (&p)[CT]) {
  static_assert(CT % 8 == 0, "class slots come in eights");
  const int C = (int)a.C;
  const Axis ax = axis_of(X, vw.sx, a.w), ay = axis_of(Y, vw.sy, a.h);
  constexpr int sh = EB == 4 ? 2 : 1;   // log2 of the element size
  const uint64_t c0 = (uint64_t)ax.i0 * a.ps0, c1 = (uint64_t)ax.i1 * a.ps0, r0 = (uint64_t)ay.i0 * a.ps1, r1 = (uint64_t)ay.i1 * a.ps1;
  const char* __restrict__ b00 = vw.src + ((c0 + r0) << sh);
  const char* __restrict__ b10 = vw.src + ((c1 + r0) << sh);
  const char* __restrict__ b01 = vw.src + ((c0 + r1) << sh);
  const char* __restrict__ b11 = vw.src + ((c1 + r1) << sh);
#pragma unroll
  for (int c = 0; c < CT; c += 8) {
    const int r = c + 8 < CT ? 8 : C - c;   // every chunk of eight but the last is full (CT - 8 < C)
    float a00[8], a10[8], a01[8], a11[8];
    load_chunk<EB>(b00 + ((size_t)c << sh), r, bf, a00);
    load_chunk<EB>(b10 + ((size_t)c << sh), r, bf, a10);
    load_chunk<EB>(b01 + ((size_t)c << sh), r, bf, a01);
    load_chunk<EB>(b11 + ((size_t)c << sh), r, bf, a11);
#pragma unroll
    for (int k = 0; k < 8; k++) p[c + k] = blend(a00[k], a10[k], a01[k], a11[k], ax.f, ay.f);
  }
  // a 16-bit source: the resampled image of the resample-then-fuse route has the source's dtype -- the same rounding, the same widening
  if constexpr (EB == 2) {
#pragma unroll
    for (int c = 0; c < CT; c++) {
      float hi;
      unpack2(bf ? bf16_rne(p[c]) : f16_rne(p[c]), bf, p[c], hi);
    }
  }
}
// The element type is a run-time, wave-uniform value: one scalar branch per pixel around the two forms of the row.
template <int CT>
__device__ __forceinline__ void sample_row(const SampArgs& a, const SampView& vw, uint32_t X, uint32_t Y, float (&p)[CT]) {
  if (a.dt == SMESH_PROBS_F32) sample_row_as<CT, 4>(a, vw, X, Y, false, p);
  else sample_row_as<CT, 2>(a, vw, X, Y, a.dt == SMESH_PROBS_BF16, p);
}

// NV views (1, 2, 4 or 8) of (w,h,C) class vectors into the accumulator in ONE launch, in order: k_fuse_tri_h16's structure.  Lane =
// triangle, wave = 64 consecutive rows parked in LDS (one round trip of the block for all views), a visible pixel's row sampled from
// the source image in registers, the float32 additions in pixel order, view 0 first -- the oracle's.  CT: class-vector register slots
// (8, 16 .. 48), the class count is a run-time value C <= CT with CT - 8 < C.  The element type is a run-time, wave-uniform value
// (SampArgs::dt): the two branches it costs per chunk are scalar, a template parameter would triple 48 instances.
// One pixel per lane is in flight (PB = 1) in every instance, and the loop over the views is a loop: the sampling code stands once per
// instance, not NV times.  No amdgpu_waves_per_eu budget: every one tried made the allocator spill (registers: DESIGN.md 3.9).
template <int CT, int KIND, int NV>
__global__ __launch_bounds__(kWave) void k_fuse_tri_sampled(SampArgs a, SampViews<NV> vw) {
  const int C = (int)a.C;
  constexpr int KV = rows_quads(CT);
  __shared__ __attribute__((aligned(16))) float srow[kWave * CT + 4];   // the wave's 64 accumulator rows
  const int l = threadIdx.x;
  if (blockIdx.x >= a.tri_blocks) {
    // (a loop over the views, not NV copies of the sampling code)
    for_each_queued_triangle<NV, false>(a, vw, blockIdx.x - a.tri_blocks, a.big_blocks,
                                        [&](const uint32_t f, const int j, const int x0, const int y0, const int x1, const int y1) __attribute__((always_inline)) {
      const SampView& view = vw.v[j];
      fuse_box_rows<CT, KIND>(a, view, f, x0, y0, x1, y1, [&](const uint32_t x, const uint32_t y, float (&p)[CT]) __attribute__((always_inline)) {
        sample_row<CT>(a, view, x, y, p);
      });
    });
    return;
  }
  const uint64_t f0 = (uint64_t)blockIdx.x * kWave;
  const uint64_t f = f0 + l;
  uint32_t org[NV];
  unsigned long long msk[NV];
  bool big;
  const unsigned long long any_win = visible_masks<NV>(a, vw, f, org, msk, big);
  if (__ballot(any_win != 0ull) == 0ull) return;   // nothing of these 64 triangles is visible: rows untouched

  // (k_fuse_tri_h16 issues the wave's 64 rows into registers together with the first pixel's loads; here four corner rows per pixel are
  // in flight already, and the block goes from memory to LDS after the first pixel's rows were asked for -- CT registers less)
  const int nrows = (int)min((uint64_t)kWave, a.F - f0);
  float* __restrict__ blk = a.acc + f0 * C;
  float accr[CT];
  bool rows_loaded = false;
#pragma nounroll
  for (int v = 0; v < NV; v++) {   // (v is wave-uniform: the view comes from the kernel arguments, this lane's origin and mask by selection)
    uint32_t o = 0u;
    unsigned long long mm = 0ull;
#pragma unroll
    for (int j = 0; j < NV; j++) if (j == v) { o = org[j]; mm = msk[j]; }
    const SampView& view = vw.v[v];
    const float* __restrict__ weights = view.weights;
    const uint32_t nv = (uint32_t)__popcll(mm);   // this primitive's pixels in this view: the histogram entry of Mesh.h:90-93
    float w0 = 0.0f;
    if (nv) {
      const float image_weight = 1.0f / ((float)nv);                         // Mesh.h:100
      const float pixel_w = 1.0f;                                            // :101
      w0 = a.iew * image_weight + (1 - a.iew) * pixel_w;                     // :102
    }
    while (__ballot(mm != 0ull) != 0ull) {
      const bool have = mm != 0ull;
      int k = 0;
      if (mm) { k = __ffsll((long long)mm) - 1; mm &= mm - 1ull; }
      const uint32_t x = (o & 0xFFFFu) + (uint32_t)(k >> 3), y = (o >> 16) + (uint32_t)(k & 7);
      float p[CT];
      // (a lane without a pixel samples the image's first pixel: unconditional, so that the loads overlap)
      sample_row<CT>(a, view, have ? x : 0u, have ? y : 0u, p);
      const float wt = (weights && have) ? weights[(uint64_t)x * view.H + y] : 1.0f;
      if (!rows_loaded) {
        // park the block in LDS (flat, coalesced) and pick up this lane's row
        if (nrows == kWave) {
          f4* s4 = reinterpret_cast<f4*>(srow);
          const f4* b4 = reinterpret_cast<const f4*>(blk);
#pragma unroll
          for (int q = 0; q < KV; q++)
            if (l + q * kWave < kWave * C / 4) s4[l + q * kWave] = b4[l + q * kWave];
        } else {
          for (int q = l; q < nrows * C; q += kWave) srow[q] = blk[q];
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < CT; c++) if (c < C) accr[c] = srow[l * C + c];
        rows_loaded = true;
      }
      // Mesh.h:94-106 for this primitive's pixels, in image order (x, then y)
      const float sum = row_sum<CT>(p, C);
      if (have && sum > 0.5f) add_pixel<CT, KIND>(p, C, w0 * wt, accr);    // :98, :103
    }
  }
  store_rows<CT>(a.acc, srow, blk, f, nrows, C, big, any_win != 0ull, accr);
}

size_t itemsize(int dt) { return dt == SMESH_PROBS_F32 ? 4 : 2; }

// The checks the entry points share.  `s`: the caller's strides or null.
int check_sampled_source(const char* who, int dt, const int64_t* s, uint64_t w, uint64_t h, int mode) {
  const std::string p = std::string(who) + ": ";
  if (dt != SMESH_PROBS_F32 && dt != SMESH_PROBS_F16 && dt != SMESH_PROBS_BF16) return fail(SMESH_ERR_INVALID, p + "bad class-vector dtype");
  if (mode != SMESH_RESIZE_BILINEAR) return fail(SMESH_ERR_INVALID, p + "unknown resampling mode");
  if (s && (s[0] < 0 || s[1] < 0 || s[2] < 0)) return fail(SMESH_ERR_INVALID, p + "negative strides are not supported");
  if (w == 0 || h == 0) return fail(SMESH_ERR_INVALID, p + "an empty source image cannot fill a view");
  if (w > 65536 || h > 65536) return fail(SMESH_ERR_INVALID, p + "source image too large");
  return SMESH_OK;
}

// Can k_fuse_tri_sampled read an image with these element strides in place?  Class stride 1 (any with one class); x and y strides fit
// the kernel's 32 bits.
bool takes_strides(const int64_t* s, uint32_t C) {
  return (s[2] == 1 || C == 1) && s[0] <= 0xFFFFFFFFll && s[1] <= 0xFFFFFFFFll;
}

}  // namespace

// ---- what raster.hip calls --------------------------------------------------------------------------------------------------

// Do sampled views rendered by a triangle renderer of F triangles in the caller's face order take k_fuse_tri_sampled for this
// aggregator?  Sum / Summax, rows in triangle order, a class count the register slots hold, and the "fuse_sampled" hook.
bool smesh_sampled_native(smesh_aggregator* a, uint64_t F) {
  int kind;
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, &kind, nullptr);
  return opt_fuse_sampled() && kind != SMESH_AGG_MUL && F != 0 && C <= kHalfMaxClasses && smesh_aggregator_can_fuse_triangles(a, F);
}

// views[v].image: the (w,h,C) source image of view v in device memory (`src`: dtype, size and strides of them all); views[v].W, H:
// the view's own size.  `nviews` = 1, 2, 4 or 8.
int smesh_sampled_fuse_triangles(smesh_aggregator* a, uint64_t F, uint32_t big_capacity, const RenderedView* views, int nviews, const SampledSrc& src) {
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  hipStream_t st = ctx->stream;
  if (F == 0) return SMESH_OK;
  SampArgs t;
  int kind;
  SMESH_TRY(check_fuse_rows("fuse_triangles_sampled", "fuse_view_sampled()", a, F, nviews, kHalfMaxClasses, &t, &kind));
  if (src.w == 0 || src.h == 0 || src.s0 < 0 || src.s1 < 0 || src.s0 > 0xFFFFFFFFll || src.s1 > 0xFFFFFFFFll)
    return fail(SMESH_ERR_INVALID, "fuse_triangles_sampled: source size or strides out of range");
  SampViews<8> tv;
  for (int v = 0; v < 8; v++) {
    const RenderedView& rv = views[v < nviews ? v : 0];
    if (rv.W == 0 || rv.H == 0 || !rv.image) return fail(SMESH_ERR_INVALID, "fuse_triangles_sampled: class-vector image missing");
    if (reinterpret_cast<uintptr_t>(rv.image) % itemsize(src.dtype)) return fail(SMESH_ERR_INVALID, "fuse_triangles_sampled: the image is not aligned to its element size");
    tv.v[v] = SampView{rv.frags, rv.idx, static_cast<const char*>(rv.image), rv.weights, rv.big_queue, rv.big_len,
                       (double)src.w / (double)rv.W, (double)src.h / (double)rv.H, (uint32_t)rv.W, (uint32_t)rv.H};
  }
  const dim3 grid = fuse_rows_grid(ctx, F, big_capacity, views, nviews, &t), block(kWave);
  t.dt = (uint32_t)src.dtype;
  t.w = src.w; t.h = src.h;
  t.ps0 = (uint32_t)src.s0; t.ps1 = (uint32_t)src.s1;
  ProfScope prof(ctx, SMESH_PROF_FUSE_SCATTER);
  prof_note(ctx, SMESH_PROF_FUSE_SCATTER, 1, (uint64_t)nviews);
  launch_fuse_rows<true>((int)((t.C + 7u) / 8u) * 8, kind, nviews, [&](auto CT, auto KIND, auto NV) {
    hipLaunchKernelGGL((k_fuse_tri_sampled<CT(), KIND(), NV()>), grid, block, 0, st, t, (first_views<SampViews, NV()>(tv)));
  });
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// ---- include/smesh_sampled.h ----------------------------------------------------------------------------------------------------
extern "C" {

int smesh_fuse_views_sampled(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* probs,
                             int probs_dtype, const int64_t probs_strides[3], uint64_t w, uint64_t h, const float* const* weights,
                             int memkind, int mode) {
  if (!r || !a || (n && (!cams || !probs))) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(check_sampled_source("fuse views sampled", probs_dtype, probs_strides, w, h, mode));
  if (memkind != SMESH_MEM_HOST && memkind != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  const size_t eb = itemsize(probs_dtype);
  bool identity = true;
  for (uint64_t i = 0; i < n; i++) {
    if (!probs[i]) return fail(SMESH_ERR_INVALID, "NULL probs image");
    if (reinterpret_cast<uintptr_t>(probs[i]) % eb) return fail(SMESH_ERR_INVALID, "fuse views sampled: an image is not aligned to its element size");
    if (cams[i].width == 0 || cams[i].height == 0 || cams[i].width > 65536 || cams[i].height > 65536)
      return fail(SMESH_ERR_INVALID, "camera resolution must be in [1, 65536]");
    identity = identity && cams[i].width == w && cams[i].height == h;
  }
  DeviceCtx* ctx = smesh_renderer_ctx(r);
  if (smesh_aggregator_ctx(a) != ctx) return fail(SMESH_ERR_INVALID, "renderer and aggregator live on different devices");
  if (n == 0) return SMESH_OK;
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  const int64_t dense3[3] = {(int64_t)(h * C), (int64_t)C, 1};
  const int64_t* ps = probs_strides ? probs_strides : dense3;
  const bool dense = ps[0] == dense3[0] && ps[1] == dense3[1] && (ps[2] == 1 || C == 1);
  if (identity && dense) {   // the views' own size: the images pass through untouched
    if (probs_dtype == SMESH_PROBS_F32) return smesh_fuse_views(r, a, cams, n, reinterpret_cast<const float* const*>(probs), weights, memkind);
    return smesh_fuse_views_probs16(r, a, cams, n, probs, probs_dtype, weights, memkind);
  }
  HalfScratch& hs = smesh_aggregator_half_scratch(a);
  std::lock_guard<std::mutex> g(hs.smp_mu);
  // (the fuse_sampled hook is read once here and again by the driver: clearing it from another thread in mid-call makes the call
  // fail with SMESH_ERR_INVALID, nothing worse -- it is a test hook, set between calls)
  const bool native = takes_strides(ps, C) && smesh_renderer_sampled_native(r, a);
  const SampledSrc src{probs_dtype, (uint32_t)w, (uint32_t)h, ps[0], ps[1]};
  const uint64_t span = source_span(ps, w, h, C);
  // one slot size for the whole call: scratch that grew between two groups would go through dev_free, which returns only when the
  // device is idle -- a device-wide wait in the middle of the group pipeline
  size_t full_bytes = 256, w_bytes = 256;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t N = cams[i].width * cams[i].height;
    full_bytes = std::max(full_bytes, round256(N * C * eb));
    w_bytes = std::max(w_bytes, round256(N * 4));
  }
  const size_t stage_bytes = round256(span * eb);
  const size_t slots = (size_t)std::min<uint64_t>(kGroup, n);
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    if (memkind == SMESH_MEM_HOST && weights) SMESH_TRY(hs.smp_w.reserve(w_bytes * slots));
    if (memkind == SMESH_MEM_HOST && native) SMESH_TRY(hs.smp_stage.reserve(stage_bytes * slots));
    if (!native) SMESH_TRY(hs.smp_full.reserve(full_bytes * slots));
  }
  // groups of up to eight views: host images cross PCIe at the source's size into the scratch, which the next group's copies
  // overwrite behind this group's fusion on the main stream
  for (uint64_t i = 0; i < n; i += kGroup) {
    const int m = (int)std::min<uint64_t>(kGroup, n - i);
    const void* dev[kGroup];
    const float* wts[kGroup];
    for (int v = 0; v < m; v++) { dev[v] = probs[i + v]; wts[v] = weights ? weights[i + v] : nullptr; }
    if (memkind == SMESH_MEM_HOST && (native || weights)) {
      std::lock_guard<std::recursive_mutex> lock(ctx->mu);
      SMESH_HIP(hipSetDevice(ctx->device));
      // (the span the strides cover, as it is: the staged image keeps its strides)
      SMESH_TRY(stage_host_group(ctx, &cams[i], m, &probs[i], weights ? &weights[i] : nullptr, native ? &hs.smp_stage : nullptr, stage_bytes,
                                 [&](int) { return (size_t)(span * eb); }, hs.smp_w, w_bytes, dev, wts));
    }
    if (native) {
      SMESH_TRY(smesh_renderer_fuse_views_sampled(r, a, &cams[i], (uint64_t)m, dev, weights ? wts : nullptr, ViewInput::sampled(nullptr, src)));
      continue;
    }
    // what the kernel does not serve: each image resampled into its scratch slot (a host image is staged and consumed by that call),
    // then the existing entry point for the group
    for (int v = 0; v < m; v++) {
      void* out = static_cast<char*>(hs.smp_full.ptr) + (size_t)v * full_bytes;
      SMESH_TRY(smesh_resize_probs(probs[i + v], probs_dtype, ps, memkind, w, h, C, out, probs_dtype, cams[i + v].width, cams[i + v].height, mode,
                                   ctx->device));
      dev[v] = out;
    }
    if (probs_dtype == SMESH_PROBS_F32)
      SMESH_TRY(smesh_fuse_views(r, a, &cams[i], (uint64_t)m, reinterpret_cast<const float* const*>(dev), weights ? wts : nullptr, SMESH_MEM_DEVICE));
    else
      SMESH_TRY(smesh_fuse_views_probs16(r, a, &cams[i], (uint64_t)m, dev, probs_dtype, weights ? wts : nullptr, SMESH_MEM_DEVICE));
  }
  return SMESH_OK;
}

int smesh_fuse_view_sampled(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cam, const void* probs, int probs_dtype,
                            const int64_t probs_strides[3], uint64_t w, uint64_t h, const float* weights, int memkind, int mode) {
  if (!cam) return fail(SMESH_ERR_INVALID, "NULL argument");
  return smesh_fuse_views_sampled(r, a, cam, 1, &probs, probs_dtype, probs_strides, w, h, weights ? &weights : nullptr, memkind, mode);
}

int smesh_aggregator_add_sampled(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                 int idx_mem, const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_mem,
                                 const float* weights, const int64_t w_strides[2], int w_mem, uint64_t w, uint64_t h, uint64_t W, uint64_t H,
                                 int mode) {
  if (!a || !indices || !probs) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (idx_dtype < 0 || idx_dtype > 3) return fail(SMESH_ERR_INVALID, "bad index dtype");
  SMESH_TRY(check_sampled_source("add sampled", probs_dtype, probs_strides, w, h, mode));
  if ((idx_strides && (idx_strides[0] < 0 || idx_strides[1] < 0)) || (weights && w_strides && (w_strides[0] < 0 || w_strides[1] < 0)))
    return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  for (int mem : {idx_mem, probs_mem, weights ? w_mem : SMESH_MEM_HOST})
    if (mem != SMESH_MEM_HOST && mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  const size_t eb = itemsize(probs_dtype);
  if (reinterpret_cast<uintptr_t>(probs) % eb) return fail(SMESH_ERR_INVALID, "add sampled: the image is not aligned to its element size");
  if (W == 0 || H == 0) return SMESH_OK;
  if (W > 65536 || H > 65536 || W * H >= 0x7FFFFFFFull / 4) return fail(SMESH_ERR_INVALID, "image too large");
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  if (r && smesh_renderer_ctx(r) != ctx) r = nullptr;
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  const uint64_t N = W * H;
  const int64_t dense2[2] = {(int64_t)H, 1};
  const int64_t dense3[3] = {(int64_t)(h * C), (int64_t)C, 1};
  const int64_t* is = idx_strides ? idx_strides : dense2;
  const int64_t* ws = w_strides ? w_strides : dense2;
  const int64_t* ps = probs_strides ? probs_strides : dense3;
  HalfScratch& hs = smesh_aggregator_half_scratch(a);
  std::lock_guard<std::mutex> g(hs.smp_mu);
  const bool w_dense = !weights || (ws[0] == (int64_t)H && ws[1] == 1);
  const bool rendered = r && idx_mem == SMESH_MEM_DEVICE && idx_dtype == SMESH_IDX_U32 && is[0] == (int64_t)H && is[1] == 1 && w_dense;
  if (rendered && takes_strides(ps, C) && smesh_renderer_sampled_native(r, a)) {
    const void* d_probs = probs;
    const float* d_w = weights;
    if (probs_mem == SMESH_MEM_HOST || (weights && w_mem == SMESH_MEM_HOST)) {
      std::lock_guard<std::recursive_mutex> lock(ctx->mu);
      SMESH_HIP(hipSetDevice(ctx->device));
      if (probs_mem == SMESH_MEM_HOST) {   // the image's span crosses PCIe as it is and keeps its strides
        const uint64_t span = source_span(ps, w, h, C);
        SMESH_TRY(hs.smp_stage.reserve(span * eb));
        SMESH_HIP(hipMemcpyAsync(hs.smp_stage.ptr, probs, span * eb, hipMemcpyHostToDevice, ctx->stream));
        d_probs = hs.smp_stage.ptr;
      }
      if (weights && w_mem == SMESH_MEM_HOST) {
        SMESH_TRY(hs.smp_w.reserve(N * 4));
        SMESH_HIP(hipMemcpyAsync(hs.smp_w.ptr, weights, N * 4, hipMemcpyHostToDevice, ctx->stream));
        d_w = static_cast<const float*>(hs.smp_w.ptr);
      }
      SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host images are consumed before the call returns
    }
    const SampledSrc src{probs_dtype, (uint32_t)w, (uint32_t)h, ps[0], ps[1]};
    int done = 0;
    SMESH_TRY(smesh_renderer_add_rendered_input(a, r, static_cast<const uint32_t*>(indices), ViewInput::sampled(d_probs, src), d_w, W, H, &done));
    if (done) return SMESH_OK;
  }
  // everything else: the image resampled on the device, then the existing entry points unchanged (asynchronous for device images)
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    SMESH_TRY(hs.smp_full.reserve(std::max<size_t>(N * C * eb, 256)));
  }
  SMESH_TRY(smesh_resize_probs(probs, probs_dtype, ps, probs_mem, w, h, C, hs.smp_full.ptr, probs_dtype, W, H, mode, ctx->device));
  const int64_t full3[3] = {(int64_t)(H * C), (int64_t)C, 1};
  if (probs_dtype != SMESH_PROBS_F32)
    return smesh_aggregator_add_probs16(a, r, indices, idx_dtype, is, idx_mem, hs.smp_full.ptr, probs_dtype, full3, SMESH_MEM_DEVICE, weights, ws, w_mem, W, H);
  const float* full = static_cast<const float*>(hs.smp_full.ptr);
  if (rendered) return smesh_aggregator_add_rendered(a, r, static_cast<const uint32_t*>(indices), full, full3, SMESH_MEM_DEVICE, weights, ws, w_mem, W, H);
  return smesh_aggregator_add_async(a, indices, idx_dtype, is, idx_mem, full, full3, SMESH_MEM_DEVICE, weights, ws, w_mem, W, H);
}

}  // extern "C"
