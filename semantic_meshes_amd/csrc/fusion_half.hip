// fusion_half.hip -- fusion of float16 / bfloat16 class-vector images without a float32 copy: the kernels, and the entry points of
// include/smesh_half.h.  A translation unit of its own: nothing here is seen by k_fuse_tri or its instance files (fuse_tri.inc.hpp is
// included for its wave helpers only, read-only).
//
// Semantics: what the float32 path gives for widen(image), where widen is exact (binary16 -> binary32 with subnormals kept; the 16
// bits of a bfloat16 become the upper half of the float32).  After the widening everything is Mesh.h:90-106 as k_fuse_tri computes it:
//     n  = pixels of p in this view's index image
//     w0 = iew * (1.0f / (float)n) + (1 - iew) * 1.0f
//     w  = w0 * weight[pixel]                       (1.0f without a weights image)
//     sum = p[0] + p[1] + ... in float32; pixels with !(sum > 0.5f) add nothing
//     Sum: acc[p][c] = acc[p][c] + p[c] * w for every c;  Summax: for c = the first largest class only
// in image order (x major, y fastest), view after view.  Mul, texel renderers, re-ordered meshes, more than kHalfMaxClasses classes and
// every image the triangle-order kernel does not serve get the image widened on the device (k_widen_probs16) and take the float32
// path unchanged.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "half_scratch.hpp"
#include "../../include/smesh_half.h"

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
int smesh_renderer_fuse_views_half(smesh_renderer* r, smesh_aggregator* a, const smesh_camera_t* cams, uint64_t n, const void* const* probs,
                                   const float* const* weights, const ViewInput& in);
int smesh_renderer_add_rendered_input(smesh_aggregator* a, smesh_renderer* r, const uint32_t* idx_dev, const ViewInput& in, const float* weights,
                                      uint64_t W, uint64_t H, int* done);

namespace {

#include "fuse_tri.inc.hpp"
#include "fuse_rows.inc.hpp"

// One view as k_fuse_tri_h16 sees it (TriView with 16-bit class vectors).
struct HalfView {
  const TriFrag* frags;
  const uint32_t* idx;
  const uint16_t* probs;      // [W][H][C] of binary16 / bfloat16 bit patterns; x and y strides ps0, ps1 in elements, class stride 1
  const float* weights;       // may be null
  const uint32_t* big_queue;
  const uint32_t* big_len;    // [0] queue length, [1] "check the masks against the index plane" flag of the render
  uint32_t W, H;
  uint32_t ps0, ps1;
};
template <int NV>
struct HalfViews {
  HalfView v[NV];
};
struct HalfFuseArgs {
  float* acc;                 // [P][C] dense
  uint64_t F;
  uint32_t C;
  float iew;
  uint32_t big_capacity;
  uint32_t tri_blocks;        // blocks 0 .. tri_blocks-1 walk the triangles, the next big_blocks the queues of triangles over 8 x 8 pixels
  uint32_t big_blocks;
  uint32_t bf16;              // nonzero: the elements are bfloat16, else binary16 (wave-uniform: one branch around the unpack)
};

// A row is 2 * C bytes at 2-byte alignment (38 bytes at 19 classes).  It is loaded in the widest pieces its length allows -- 16 bytes
// per eight classes, then 8, 4 and 2 for what is left (load_part16) -- through fuse_rows.inc.hpp's pointer types.
// The row at `pr` into CT float32 registers, C <= CT run-time classes with CT = the multiple of eight at or above C: every chunk of
// eight but the last is full.  Elements c >= C come out as +0.
template <int CT>
__device__ __forceinline__ void load_row16(const uint16_t* __restrict__ pr, int C, bool bf, float (&p)[CT]) {
  static_assert(CT % 8 == 0, "class slots come in eights");
  uint32_t w[CT / 2];
#pragma unroll
  for (int c = 0; c + 8 < CT; c += 8) {
    const u32x4 q = *reinterpret_cast<const u32x4_a2*>(pr + c);
    w[c / 2] = q.x; w[c / 2 + 1] = q.y; w[c / 2 + 2] = q.z; w[c / 2 + 3] = q.w;
  }
  constexpr int L = CT - 8;   // the last chunk: C - L = 1 .. 8 elements
  if (C == CT) {
    const u32x4 q = *reinterpret_cast<const u32x4_a2*>(pr + L);
    w[L / 2] = q.x; w[L / 2 + 1] = q.y; w[L / 2 + 2] = q.z; w[L / 2 + 3] = q.w;
  } else {
    const u32x4 q = load_part16(pr + L, C - L);   // 1 .. 7 elements (wave-uniform)
    w[L / 2] = q.x; w[L / 2 + 1] = q.y; w[L / 2 + 2] = q.z; w[L / 2 + 3] = q.w;
  }
#pragma unroll
  for (int c = 0; c < CT; c += 2) unpack2(w[c / 2], bf, p[c], p[c + 1]);
}

// NV views (1, 2, 4 or 8) of 16-bit class vectors into the accumulator in ONE launch, in order: k_fuse_tri's structure.  Lane =
// triangle, wave = 64 consecutive rows parked in LDS (one round trip of the block for all views), a visible pixel's row loaded at 16
// bits and widened in registers, the float32 additions in pixel order, view 0 first -- the oracle's.  CT: class-vector register slots
// (8, 16 .. 48), the class count is a run-time value C <= CT with CT - 8 < C.
// (Register budget, measured at cfg2's geometry with 16 views per call: left to the scheduler with two pixels in flight the 24-slot
// eight-view instance took 190 VGPRs -- two waves per SIMD -- and 40.5 us per view at 19 classes against k_fuse_tri's 34.8; with one
// pixel in flight and a budget of three waves it takes 144, no scratch, and 31.4.  As for k_fuse_tri's 19 .. 21-class instances the
// third wave is what counts; the other slots are left to the scheduler.)
constexpr int fuse_h16_min_waves(int ct) { return ct == 24 ? 3 : 1; }
template <int CT, int KIND, int NV>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(fuse_h16_min_waves(CT)))) void k_fuse_tri_h16(HalfFuseArgs a, HalfViews<NV> vw) {
  const int C = (int)a.C;
  constexpr int PB = CT <= 16 ? 2 : 1;        // pixels whose class vectors are in flight together (k_fuse_tri: two up to 24 slots; here see the budget above)
  constexpr int KV = rows_quads(CT);
  __shared__ __attribute__((aligned(16))) float srow[kWave * CT + 4];   // the wave's 64 accumulator rows
  const int l = threadIdx.x;
  const bool bf = a.bf16 != 0u;
  if (blockIdx.x >= a.tri_blocks) {
    for_each_queued_triangle<NV, true>(a, vw, blockIdx.x - a.tri_blocks, a.big_blocks,
                                       [&](const uint32_t f, const int j, const int x0, const int y0, const int x1, const int y1) __attribute__((always_inline)) {
      const HalfView& view = vw.v[j];
      fuse_box_rows<CT, KIND>(a, view, f, x0, y0, x1, y1, [&](const uint32_t x, const uint32_t y, float (&p)[CT]) __attribute__((always_inline)) {
        load_row16<CT>(view.probs + ((uint64_t)x * view.ps0 + (uint64_t)y * view.ps1), C, bf, p);
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

  // ---- issue together: the wave's 64 accumulator rows (one contiguous block) and the first PB pixels' class vectors of every lane
  const int nrows = (int)min((uint64_t)kWave, a.F - f0);
  float* __restrict__ blk = a.acc + f0 * C;
  f4 br[KV];
  if (nrows == kWave) {
    const f4* b4 = reinterpret_cast<const f4*>(blk);
#pragma unroll
    for (int q = 0; q < KV; q++) br[q] = b4[min(l + q * kWave, kWave * C / 4 - 1)];
  }
  float accr[CT];
  bool rows_loaded = false;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const uint16_t* __restrict__ probs = vw.v[v].probs;
    const float* __restrict__ weights = vw.v[v].weights;
    const uint32_t nv = (uint32_t)__popcll(msk[v]);   // this primitive's pixels in this view: the histogram entry of Mesh.h:90-93
    float w0 = 0.0f;
    if (nv) {
      const float image_weight = 1.0f / ((float)nv);                         // Mesh.h:100
      const float pixel_w = 1.0f;                                            // :101
      w0 = a.iew * image_weight + (1 - a.iew) * pixel_w;                     // :102
    }
    unsigned long long mm = msk[v];
    while (__ballot(mm != 0ull) != 0ull) {
      float p[PB][CT];
      float wt[PB];
      bool have[PB];
#pragma unroll
      for (int j = 0; j < PB; j++) {
        have[j] = mm != 0ull;
        int k = 0;
        if (mm) { k = __ffsll((long long)mm) - 1; mm &= mm - 1ull; }
        const uint32_t x = (org[v] & 0xFFFFu) + (uint32_t)(k >> 3), y = (org[v] >> 16) + (uint32_t)(k & 7);
        // (a lane without a pixel reads the image's first row: unconditional, so that the loads overlap)
        const uint16_t* __restrict__ pr = probs + (have[j] ? (uint64_t)x * vw.v[v].ps0 + (uint64_t)y * vw.v[v].ps1 : 0);
        load_row16<CT>(pr, C, bf, p[j]);
        wt[j] = (weights && have[j]) ? weights[(uint64_t)x * vw.v[v].H + y] : 1.0f;
      }
      if (!rows_loaded) {
        // park the block in LDS (flat, coalesced) and pick up this lane's row
        if (nrows == kWave) {
          f4* s4 = reinterpret_cast<f4*>(srow);
#pragma unroll
          for (int q = 0; q < KV; q++)
            if (l + q * kWave < kWave * C / 4) s4[l + q * kWave] = br[q];
        } else {
          for (int q = l; q < nrows * C; q += kWave) srow[q] = blk[q];
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < CT; c++) if (c < C) accr[c] = srow[l * C + c];
        rows_loaded = true;
      }
      // Mesh.h:94-106 for this primitive's pixels, in image order (x, then y)
#pragma unroll
      for (int j = 0; j < PB; j++) {
        const float sum = row_sum<CT>(p[j], C);
        if (have[j] && sum > 0.5f) add_pixel<CT, KIND>(p[j], C, w0 * wt[j], accr);    // :98, :103
      }
    }
  }
  store_rows<CT>(a.acc, srow, blk, f, nrows, C, big, any_win != 0ull, accr);
}

// Any strided (W,H,C) 16-bit image -> the dense float32 one the float32 kernels read.  DENSE (class stride 1, rows back to back):
// eight elements per thread, one 16-byte load and two 16-byte stores; else element by element (a route for odd layouts, no speed claimed).
template <bool DENSE>
__global__ __launch_bounds__(256) void k_widen_probs16(const uint16_t* __restrict__ in, int64_t s0, int64_t s1, int64_t s2, float* __restrict__ out,
                                                       uint64_t total, uint32_t H, uint32_t C, uint32_t bf16) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bf = bf16 != 0u;
  if (DENSE) {
    const uint64_t e = t * 8u;
    if (e >= total) return;
    if (e + 8u <= total) {
      const u32x4 q = *reinterpret_cast<const u32x4_a2*>(in + e);
      float v[8];
      unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]); unpack2(q.z, bf, v[4], v[5]); unpack2(q.w, bf, v[6], v[7]);
      fvec4 o0, o1;
      o0.x = v[0]; o0.y = v[1]; o0.z = v[2]; o0.w = v[3];
      o1.x = v[4]; o1.y = v[5]; o1.z = v[6]; o1.w = v[7];
      *reinterpret_cast<fvec4_a4*>(out + e) = o0;
      *reinterpret_cast<fvec4_a4*>(out + e + 4) = o1;
    } else {
      for (uint64_t i = e; i < total; i++) {
        float lo, hi;
        unpack2((uint32_t)in[i], bf, lo, hi);
        out[i] = lo;
      }
    }
  } else {
    if (t >= total) return;
    const uint64_t pix = t / C, c = t - pix * C;
    const uint64_t x = pix / H, y = pix - x * H;
    float lo, hi;
    unpack2((uint32_t)in[x * (uint64_t)s0 + y * (uint64_t)s1 + c * (uint64_t)s2], bf, lo, hi);
    out[t] = lo;
  }
}

// (bf16_rne / f16_rne, the narrowing of smesh_narrow_probs: half_scratch.hpp)
// smesh_narrow_probs: four elements per thread (one 16-byte load, one 8-byte store), the last few one by one.
__global__ __launch_bounds__(256) void k_narrow_probs(const float* __restrict__ in, uint16_t* __restrict__ out, uint64_t n, uint32_t bf16) {
  const uint64_t e = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4u;
  if (e >= n) return;
  if (e + 4u <= n) {
    const fvec4 q = *reinterpret_cast<const fvec4_a4*>(in + e);
    u32x2 o;
    if (bf16) { o.x = bf16_rne(q.x) | (bf16_rne(q.y) << 16); o.y = bf16_rne(q.z) | (bf16_rne(q.w) << 16); }
    else { o.x = f16_rne(q.x) | (f16_rne(q.y) << 16); o.y = f16_rne(q.z) | (f16_rne(q.w) << 16); }
    *reinterpret_cast<u32x2_a2*>(out + e) = o;
  } else {
    for (uint64_t i = e; i < n; i++) out[i] = (uint16_t)(bf16 ? bf16_rne(in[i]) : f16_rne(in[i]));
  }
}

int check_half_dtype(int dt) {
  if (dt == SMESH_PROBS_F16 || dt == SMESH_PROBS_BF16) return SMESH_OK;
  if (dt == SMESH_PROBS_F32) return fail(SMESH_ERR_INVALID, "SMESH_PROBS_F32: float32 class vectors go through the entry points of smesh.h");
  return fail(SMESH_ERR_INVALID, "bad probs dtype");
}

// Test hook SMESH_FUSE_H16=0: every 16-bit image takes the widening route.  Read at every call (one getenv beside a kernel launch), so
// that tools/half_probs_bench.py measures both routes in one process.
bool h16_enabled() { return env_int("SMESH_FUSE_H16", 1) != 0; }

}  // namespace

// ---- what raster.hip calls --------------------------------------------------------------------------------------------------

// Do 16-bit views rendered by a triangle renderer of F triangles in the caller's face order take k_fuse_tri_h16 for this aggregator?
// Sum / Summax, rows in triangle order, a class count the register slots hold.
bool smesh_half_native(smesh_aggregator* a, uint64_t F) {
  int kind;
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, &kind, nullptr);
  return h16_enabled() && kind != SMESH_AGG_MUL && F != 0 && C <= kHalfMaxClasses && smesh_aggregator_can_fuse_triangles(a, F);
}

// Can k_fuse_tri_h16 read an image with these element strides in place?  (Class stride 1; x and y strides fit the kernel's 32 bits.)
bool smesh_half_takes_strides(int64_t ps0, int64_t ps1) { return ps0 > 0 && ps1 > 0 && ps0 <= 0xFFFFFFFFll && ps1 <= 0xFFFFFFFFll; }

// views[v].image: (W,H,C) images of `probs_dtype` in device memory, x / y strides views[v].ps0 / ps1 (0, 0: dense).  `nviews` = 1, 2, 4 or 8.
int smesh_half_fuse_triangles(smesh_aggregator* a, uint64_t F, uint32_t big_capacity, const RenderedView* views, int nviews, int probs_dtype) {
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  hipStream_t st = ctx->stream;
  if (F == 0) return SMESH_OK;
  HalfFuseArgs t;
  int kind;
  SMESH_TRY(check_half_dtype(probs_dtype));
  SMESH_TRY(check_fuse_rows("fuse_triangles_half", "fuse_view_probs16()", a, F, nviews, kHalfMaxClasses, &t, &kind));
  HalfViews<8> tv;
  for (int v = 0; v < 8; v++) {
    const RenderedView& rv = views[v < nviews ? v : 0];
    if (rv.W == 0 || rv.H == 0 || !rv.image) return fail(SMESH_ERR_INVALID, "fuse_triangles_half: class-vector image missing");
    if (reinterpret_cast<uintptr_t>(rv.image) & 1) return fail(SMESH_ERR_INVALID, "fuse_triangles_half: 16-bit class vectors must be 2-byte aligned");
    const int64_t ps0 = (rv.ps0 || rv.ps1) ? rv.ps0 : (int64_t)(rv.H * t.C), ps1 = (rv.ps0 || rv.ps1) ? rv.ps1 : (int64_t)t.C;
    if (!smesh_half_takes_strides(ps0, ps1)) return fail(SMESH_ERR_INVALID, "fuse_triangles_half: class-vector strides out of range");
    tv.v[v] = HalfView{rv.frags, rv.idx, static_cast<const uint16_t*>(rv.image), rv.weights, rv.big_queue, rv.big_len,
                       (uint32_t)rv.W, (uint32_t)rv.H, (uint32_t)ps0, (uint32_t)ps1};
  }
  const dim3 grid = fuse_rows_grid(ctx, F, big_capacity, views, nviews, &t), block(kWave);
  t.bf16 = probs_dtype == SMESH_PROBS_BF16 ? 1u : 0u;
  ProfScope prof(ctx, SMESH_PROF_FUSE_SCATTER);
  prof_note(ctx, SMESH_PROF_FUSE_SCATTER, 1, (uint64_t)nviews);
  launch_fuse_rows<true>((int)((t.C + 7u) / 8u) * 8, kind, nviews, [&](auto CT, auto KIND, auto NV) {
    hipLaunchKernelGGL((k_fuse_tri_h16<CT(), KIND(), NV()>), grid, block, 0, st, t, (first_views<HalfViews, NV()>(tv)));
  });
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// The widening route's class vectors: a strided (W,H,C) device image of `probs_dtype` (element strides s[3]) as dense float32 in the
// aggregator's scratch, on the main stream: slot `slot` of `nslots` slots `slot_bytes` apart (the images of a group of views; 0: one
// image).  One buffer: whoever reads it is queued on that stream before the next widening into the same slot.
int smesh_half_widen(smesh_aggregator* a, const void* probs, int probs_dtype, const int64_t s[3], uint64_t W, uint64_t H, const float** out,
                     int slot, size_t slot_bytes, int nslots) {
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  HalfScratch& hs = smesh_aggregator_half_scratch(a);
  SMESH_TRY(check_half_dtype(probs_dtype));
  if (reinterpret_cast<uintptr_t>(probs) & 1) return fail(SMESH_ERR_INVALID, "16-bit class vectors must be 2-byte aligned");
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  const uint64_t total = W * H * C;
  if (slot_bytes == 0) { slot = 0; nslots = 1; slot_bytes = std::max<uint64_t>(total * 4, 16); }
  if (slot < 0 || slot >= nslots || total * 4 > slot_bytes) return fail(SMESH_ERR_INVALID, "widen: bad scratch slot");
  SMESH_TRY(hs.wide.reserve(slot_bytes * (size_t)nslots));
  float* dst = reinterpret_cast<float*>(static_cast<char*>(hs.wide.ptr) + (size_t)slot * slot_bytes);
  if (total) {
    const bool dense = (s[2] == 1 || C == 1) && (s[1] == (int64_t)C || H == 1) && (s[0] == (int64_t)(H * C) || W == 1);
    const uint32_t bf = probs_dtype == SMESH_PROBS_BF16 ? 1u : 0u;
    const dim3 b(256);
    if (dense) hipLaunchKernelGGL(k_widen_probs16<true>, dim3((uint32_t)div_up(div_up(total, 8), 256)), b, 0, ctx->stream,
                                  static_cast<const uint16_t*>(probs), s[0], s[1], s[2], dst, total, (uint32_t)H, C, bf);
    else hipLaunchKernelGGL(k_widen_probs16<false>, dim3((uint32_t)div_up(total, 256)), b, 0, ctx->stream,
                            static_cast<const uint16_t*>(probs), s[0], s[1], s[2], dst, total, (uint32_t)H, C, bf);
    SMESH_HIP(hipGetLastError());
  }
  *out = dst;
  return SMESH_OK;
}

// ---- include/smesh_half.h -------------------------------------------------------------------------------------------------------
extern "C" {

int smesh_fuse_views_probs16(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* probs,
                             int probs_dtype, const float* const* weights, int memkind) {
  if (!r || !a || (n && (!cams || !probs))) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(check_half_dtype(probs_dtype));
  if (memkind != SMESH_MEM_HOST && memkind != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  for (uint64_t i = 0; i < n; i++) {
    if (!probs[i]) return fail(SMESH_ERR_INVALID, "NULL probs image");
    if (reinterpret_cast<uintptr_t>(probs[i]) & 1) return fail(SMESH_ERR_INVALID, "16-bit class vectors must be 2-byte aligned");
    if (cams[i].width == 0 || cams[i].height == 0 || cams[i].width > 65536 || cams[i].height > 65536)
      return fail(SMESH_ERR_INVALID, "camera resolution must be in [1, 65536]");
  }
  DeviceCtx* ctx = smesh_renderer_ctx(r);
  if (smesh_aggregator_ctx(a) != ctx) return fail(SMESH_ERR_INVALID, "renderer and aggregator live on different devices");
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  HalfScratch& hs = smesh_aggregator_half_scratch(a);
  std::lock_guard<std::mutex> g(hs.mu);
  if (memkind == SMESH_MEM_DEVICE) return smesh_renderer_fuse_views_half(r, a, cams, n, probs, weights, ViewInput::half(nullptr, probs_dtype));
  // host images, in groups of up to eight views: they cross PCIe at 16 bits into the scratch, which the next group's copies overwrite
  // behind this group's fusion on the main stream
  for (uint64_t i = 0; i < n; i += kGroup) {
    const int m = (int)std::min<uint64_t>(kGroup, n - i);
    size_t slot_bytes = 0, w_bytes = 0;
    for (int v = 0; v < m; v++) {
      const uint64_t N = cams[i + v].width * cams[i + v].height;
      slot_bytes = std::max(slot_bytes, round256(N * C * 2));
      w_bytes = std::max(w_bytes, round256(N * 4));
    }
    const void* dev[kGroup];
    const float* wts[kGroup];
    {
      std::lock_guard<std::recursive_mutex> lock(ctx->mu);
      SMESH_HIP(hipSetDevice(ctx->device));
      SMESH_TRY(hs.stage.reserve(slot_bytes * (size_t)m));
      if (weights) SMESH_TRY(hs.w.reserve(w_bytes * (size_t)m));
      SMESH_TRY(stage_host_group(ctx, &cams[i], m, &probs[i], weights ? &weights[i] : nullptr, &hs.stage, slot_bytes,
                                 [&](int v) { return (size_t)(cams[i + v].width * cams[i + v].height * C * 2); }, hs.w, w_bytes, dev, wts));
    }
    SMESH_TRY(smesh_renderer_fuse_views_half(r, a, &cams[i], (uint64_t)m, dev, weights ? wts : nullptr, ViewInput::half(nullptr, probs_dtype)));
  }
  return SMESH_OK;
}

int smesh_fuse_view_probs16(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cam, const void* probs, int probs_dtype,
                            const float* weights, int memkind) {
  if (!cam) return fail(SMESH_ERR_INVALID, "NULL argument");
  return smesh_fuse_views_probs16(r, a, cam, 1, &probs, probs_dtype, weights ? &weights : nullptr, memkind);
}

int smesh_aggregator_add_probs16(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                 int idx_mem, const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_mem,
                                 const float* weights, const int64_t w_strides[2], int w_mem, uint64_t W, uint64_t H) {
  if (!a || !indices || !probs) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (idx_dtype < 0 || idx_dtype > 3) return fail(SMESH_ERR_INVALID, "bad index dtype");
  SMESH_TRY(check_half_dtype(probs_dtype));
  if ((idx_strides && (idx_strides[0] < 0 || idx_strides[1] < 0)) || (weights && w_strides && (w_strides[0] < 0 || w_strides[1] < 0)) ||
      (probs_strides && (probs_strides[0] < 0 || probs_strides[1] < 0 || probs_strides[2] < 0)))
    return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  for (int mem : {idx_mem, probs_mem, weights ? w_mem : SMESH_MEM_HOST})
    if (mem != SMESH_MEM_HOST && mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (reinterpret_cast<uintptr_t>(probs) & 1) return fail(SMESH_ERR_INVALID, "16-bit class vectors must be 2-byte aligned");
  if (W == 0 || H == 0) return SMESH_OK;
  if (W > 65536 || H > 65536 || W * H >= 0x7FFFFFFFull / 4) return fail(SMESH_ERR_INVALID, "image too large");
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  if (r && smesh_renderer_ctx(r) != ctx) r = nullptr;
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  const uint64_t N = W * H;
  const int64_t dense2[2] = {(int64_t)H, 1};
  const int64_t dense3[3] = {(int64_t)(H * C), (int64_t)C, 1};
  const int64_t* is = idx_strides ? idx_strides : dense2;
  const int64_t* ws = w_strides ? w_strides : dense2;
  const int64_t* ps = probs_strides ? probs_strides : dense3;
  HalfScratch& hs = smesh_aggregator_half_scratch(a);
  std::lock_guard<std::mutex> g(hs.mu);
  const void* d_probs = probs;
  const float* d_w = weights;
  const bool w_dense = !weights || (ws[0] == (int64_t)H && ws[1] == 1);
  const bool rendered = r && idx_mem == SMESH_MEM_DEVICE && idx_dtype == SMESH_IDX_U32 && is[0] == (int64_t)H && is[1] == 1 && w_dense;
  if (probs_mem == SMESH_MEM_HOST || (rendered && weights && w_mem == SMESH_MEM_HOST)) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    if (probs_mem == SMESH_MEM_HOST) {   // the image's span crosses PCIe as it is, at 16 bits, and keeps its strides
      const uint64_t span = source_span(ps, W, H, C);
      SMESH_TRY(hs.stage.reserve(span * 2));
      SMESH_HIP(hipMemcpyAsync(hs.stage.ptr, probs, span * 2, hipMemcpyHostToDevice, ctx->stream));
      d_probs = hs.stage.ptr;
    }
    if (rendered && weights && w_mem == SMESH_MEM_HOST) {   // (the triangle-order kernel wants the weights where the image is)
      SMESH_TRY(hs.w.reserve(N * 4));
      SMESH_HIP(hipMemcpyAsync(hs.w.ptr, weights, N * 4, hipMemcpyHostToDevice, ctx->stream));
      d_w = static_cast<const float*>(hs.w.ptr);
    }
    SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host images are consumed before the call returns
  }
  if (rendered && (ps[2] == 1 || C == 1) && smesh_half_takes_strides(ps[0], ps[1])) {
    int done = 0;
    SMESH_TRY(smesh_renderer_add_rendered_input(a, r, static_cast<const uint32_t*>(indices), ViewInput::half(d_probs, probs_dtype, ps[0], ps[1]), d_w, W, H, &done));
    if (done) return SMESH_OK;
  }
  // everything else: the image widened on the device, then the float32 path unchanged (asynchronous for device images)
  const float* wide = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    SMESH_TRY(smesh_half_widen(a, d_probs, probs_dtype, ps, W, H, &wide, 0, 0, 1));
  }
  return smesh_aggregator_add_async(a, indices, idx_dtype, is, idx_mem, wide, dense3, SMESH_MEM_DEVICE, weights, ws, w_mem, W, H);
}

int smesh_narrow_probs(const float* in, void* out, uint64_t n, int probs_dtype, int device, int memkind) {
  SMESH_TRY(check_half_dtype(probs_dtype));
  if (memkind != SMESH_MEM_HOST && memkind != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (n == 0) return SMESH_OK;
  if (!in || !out) return fail(SMESH_ERR_INVALID, "NULL argument");
  if ((reinterpret_cast<uintptr_t>(in) & 3) || (reinterpret_cast<uintptr_t>(out) & 1)) return fail(SMESH_ERR_INVALID, "misaligned argument");
  if (n > (uint64_t)0x7FFFFFFF * 1024u) return fail(SMESH_ERR_INVALID, "too many elements");
  DeviceCtx* ctx;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const uint32_t bf = probs_dtype == SMESH_PROBS_BF16 ? 1u : 0u;
  const dim3 grid((uint32_t)div_up(div_up(n, 4), 256)), block(256);
  if (memkind == SMESH_MEM_DEVICE) {
    hipLaunchKernelGGL(k_narrow_probs, grid, block, 0, ctx->stream, in, static_cast<uint16_t*>(out), n, bf);
    SMESH_HIP(hipGetLastError());
    return SMESH_OK;
  }
  void* d = nullptr;   // host arrays: through one device block, float32 in front, the 16-bit result behind it
  SMESH_HIP(dev_malloc(&d, n * 6));
  float* d_in = static_cast<float*>(d);
  uint16_t* d_out = reinterpret_cast<uint16_t*>(d_in + n);
  hipError_t e = hipMemcpyAsync(d_in, in, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_narrow_probs, grid, block, 0, ctx->stream, d_in, d_out, n, bf);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n * 2, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)dev_free(d);
  if (e != hipSuccess) return fail_hip(e, "smesh_narrow_probs", __FILE__, __LINE__);
  return SMESH_OK;
}

}  // extern "C"
