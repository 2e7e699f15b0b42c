// fusion_labels.hip -- fusion of LABEL images (one class index per pixel) instead of class vectors: the kernels, and the entry points of
// include/smesh_labels.h.  A translation unit of its own: nothing here is seen by k_fuse_tri or its instance files (fuse_tri.inc.hpp is
// included for its wave helpers only, read-only).
//
// Semantics: what the class-vector path gives for one_hot(labels), tf.one_hot's rule (a label outside [0, C) is the all-zero vector).
// For a pixel of primitive p with label c in range, Mesh.h:90-106 and Fusion.cu:46-76 come down to
//     n  = pixels of p in this view's index image (don't-care pixels count)
//     w0 = iew * (1.0f / (float)n) + (1 - iew) * 1.0f
//     w  = w0 * weight[pixel]                       (1.0f without a weights image)
//     acc[p][c] = acc[p][c] + 1.0f * w
// in image order (x major, y fastest), view after view -- for Sum AND Summax (the arg-max of a one-hot row is its label).  Mul and every
// renderer / image the triangle-order kernel does not serve get the labels expanded on the device (k_labels_onehot) and take the
// class-vector path unchanged.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "labels_scratch.hpp"
#include "view_input.hpp"
#include "../../include/smesh_labels.h"
#include "../../include/smesh_label_prep.h"
#include "../../include/smesh_label_colors.h"

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
LabelScratch& smesh_aggregator_label_scratch(smesh_aggregator* a);
// raster.hip
struct smesh_renderer;
DeviceCtx* smesh_renderer_ctx(smesh_renderer* r);
void smesh_set_last_fuse_instance(int slot, int views);
void smesh_note_fuse_rows_views(DeviceCtx* ctx, const RenderedView* views, int nviews);
int smesh_renderer_fuse_views_labels(smesh_renderer* r, smesh_aggregator* a, const smesh_camera_t* cams, uint64_t n, const void* const* planes,
                                     const float* const* weights, const ViewInput& in);
int smesh_renderer_add_rendered_input(smesh_aggregator* a, smesh_renderer* r, const uint32_t* idx_dev, const ViewInput& in, const float* weights,
                                      uint64_t W, uint64_t H, int* done);

namespace {

#include "fuse_tri.inc.hpp"
#include "fuse_rows.inc.hpp"

// (kLabelsLdsMaxC, the class count up to which the main waves keep their rows in LDS: labels_scratch.hpp)

// One view as k_fuse_tri_labels sees it (TriView with a label plane in place of the class vectors).
struct LabelView {
  const TriFrag* frags;
  const uint32_t* idx;
  const void* labels;         // [W][H] of LT, dense; any value >= C is "don't care"
  const float* weights;       // may be null
  const uint32_t* big_queue;
  const uint32_t* big_len;    // [0] queue length, [1] "check the masks against the index plane" flag of the render
  uint32_t W, H;
};
template <int NV>
struct LabelViews {
  LabelView v[NV];
};
struct LabelFuseArgs {
  float* acc;                 // [P][C] dense
  uint64_t F;
  uint32_t C;
  float iew;
  uint32_t big_capacity;
  uint32_t tri_blocks;        // blocks 0 .. tri_blocks-1 walk the triangles, the next big_blocks the queues of triangles over 8 x 8 pixels
  uint32_t big_blocks;
  uint32_t stride;            // IN_LDS: floats between two rows of the LDS block (C | 1)
};

// Eight consecutive labels (a column of a triangle's 8 x 8 box: y is the fastest axis) in one load at element alignment.
typedef uint64_t u64_a1 __attribute__((aligned(1)));
typedef uint64_t u64_a2 __attribute__((aligned(2)));
template <typename LT>
struct LabelRun;
template <>
struct LabelRun<uint8_t> {
  uint64_t q;
  __device__ __forceinline__ void load(const uint8_t* p) { q = *reinterpret_cast<const u64_a1*>(p); }
  __device__ __forceinline__ uint32_t pick(uint32_t i) const { return (uint32_t)(q >> (8u * i)) & 0xFFu; }
};
template <>
struct LabelRun<uint16_t> {
  uint64_t lo, hi;
  __device__ __forceinline__ void load(const uint16_t* p) {
    lo = *reinterpret_cast<const u64_a2*>(p);
    hi = *reinterpret_cast<const u64_a2*>(p + 4);
  }
  __device__ __forceinline__ uint32_t pick(uint32_t i) const { return (uint32_t)((i < 4u ? lo : hi) >> (16u * (i & 3u))) & 0xFFFFu; }
};

// One queued triangle `f` in view `vw` (for_each_queued_triangle): lanes go over the box [x0, x1] x [y0, y1] of the view's index plane.
// IN_LDS: the view's hits go to a C-float LDS histogram by LDS float adds, which lane c then adds to element c of the row; else by
// float atomics to the row itself.  Either way a tree / atomic order: the 1e-5 path, like fuse_box.
template <typename LT, bool IN_LDS>
__device__ __forceinline__ void fuse_box_labels(const LabelFuseArgs& a, const LabelView& vw, const uint32_t f, const int x0, const int y0, const int x1,
                                                const int y1, float* __restrict__ hist) {
  const int l = threadIdx.x;
  const uint32_t C = a.C;
  float* __restrict__ row = a.acc + (uint64_t)f * C;
  const uint32_t H = vw.H;
  const uint32_t bh = (uint32_t)(y1 - y0 + 1);
  const uint32_t npx = (uint32_t)(x1 - x0 + 1) * bh;
  const uint32_t* __restrict__ idx = vw.idx;
  auto pix_of = [&](uint32_t i) -> uint64_t { return (uint64_t)((uint32_t)x0 + i / bh) * H + ((uint32_t)y0 + i % bh); };
  uint32_t cnt = 0;
  for (uint32_t i = l; i < npx; i += kWave) cnt += idx[pix_of(i)] == f ? 1u : 0u;
  const uint32_t n = wave_sum_u(cnt);
  if (n == 0) return;
  const float w0 = a.iew * (1.0f / (float)n) + (1 - a.iew) * 1.0f;
  const LT* __restrict__ lab = static_cast<const LT*>(vw.labels);
  const float* __restrict__ wts = vw.weights;
  if (IN_LDS) {
    for (uint32_t c = l; c < C; c += kWave) hist[c] = 0.0f;
    wave_sync();
  }
  for (uint32_t i = l; i < npx; i += kWave) {
    const uint64_t pix = pix_of(i);
    if (idx[pix] != f) continue;
    const uint32_t c = (uint32_t)lab[pix];
    if (c >= C) continue;
    const float w = w0 * (wts ? wts[pix] : 1.0f);
    if (IN_LDS) __hip_atomic_fetch_add(&hist[c], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else unsafeAtomicAdd(&row[c], w);
  }
  if (IN_LDS) {
    wave_sync();
    for (uint32_t c = l; c < C; c += kWave) {
      const float h = hist[c];
      if (h != 0.0f) row[c] = row[c] + h;
    }
    wave_sync();   // the histogram is cleared for this wave's next view
  }
}

// NV views (1, 2, 4 or 8) of label planes into the accumulator in ONE launch, in order.  Lane = triangle, wave = 64 consecutive rows, as
// k_fuse_tri; the class count is a run-time value.  IN_LDS: the wave's 64 x C block is streamed into LDS with 16-byte loads (rows
// `stride` floats apart) and a visible pixel is ONE LDS read-modify-write at row[label] -- in pixel order, view 0 first, so the float32
// additions are the oracle's -- and the block goes back once for all views.  !IN_LDS: the same read-modify-write on the row in global
// memory (its one owner is this lane).  Labels: a triangle's <= 8 x 8 box is up to eight runs of <= 8 consecutive labels; the runs of
// a view are loaded together, one load each, and the labels picked out of them.
template <typename LT, int NV, bool IN_LDS>
__global__ __launch_bounds__(kWave) void k_fuse_tri_labels(LabelFuseArgs a, LabelViews<NV> vw) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  const int l = threadIdx.x;
  const uint32_t C = a.C;
  if (blockIdx.x >= a.tri_blocks) {
    for_each_queued_triangle<NV, true>(a, vw, blockIdx.x - a.tri_blocks, a.big_blocks,
                                       [&](const uint32_t f, const int j, const int x0, const int y0, const int x1, const int y1) __attribute__((always_inline)) {
      fuse_box_labels<LT, IN_LDS>(a, vw.v[j], f, x0, y0, x1, y1, srow);
    });
    return;
  }
  const uint64_t f0 = (uint64_t)blockIdx.x * kWave;
  const uint64_t f = f0 + l;
  // (the prologue of fuse_rows.inc.hpp's visible_masks, written out: as that helper it costs this kernel's eight-view instances 50 more
  // SGPRs spilled into VGPR lanes -- 133 against 82 -- and 5 % of the kernel's time on cfg2, profiles/fuse_rows_refactor.md)
  // per view: box origin (x0 | y0 << 16) and the mask of this triangle's VISIBLE pixels inside its <= 8 x 8 box
  uint32_t org[NV];
  unsigned long long msk[NV];
  bool big = false;   // a box over 8 x 8 in some view: the triangle is a tail wave's for all its views, and so is its row
#pragma unroll
  for (int v = 0; v < NV; v++) { org[v] = 0u; msk[v] = 0ull; }
  if (f < a.F) {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const TriFrag rec = vw.v[v].frags[f];
      org[v] = (uint32_t)rec.x0 | ((uint32_t)rec.y0 << 16);
      msk[v] = rec.kind == 1 ? rec.mask : 0ull;
      big = big || rec.kind == 2;
    }
  }
  if (big) {
#pragma unroll
    for (int v = 0; v < NV; v++) msk[v] = 0ull;
  }
  // the masks of a view whose render says they need checking (fragment-queue overflow, direct rasteriser) are checked against that
  // view's index plane, which such a view always writes (k_fuse_tri's pass 1)
#pragma unroll
  for (int v = 0; v < NV; v++) {
    if (vw.v[v].big_len[1] == 0u) continue;
    const uint32_t* __restrict__ idx = vw.v[v].idx;
    unsigned long long m = msk[v], win = 0ull;
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      const uint64_t pix = (uint64_t)((org[v] & 0xFFFFu) + (uint32_t)(k >> 3)) * vw.v[v].H + (org[v] >> 16) + (uint32_t)(k & 7);
      if (idx[pix] == (uint32_t)f) win |= 1ull << k;
    }
    msk[v] = win;
  }
  unsigned long long any_win = 0ull;
#pragma unroll
  for (int v = 0; v < NV; v++) any_win |= msk[v];
  if (__ballot(any_win != 0ull) == 0ull) return;   // nothing of these 64 triangles is visible: rows untouched

  const uint32_t S = a.stride;
  const int nrows = (int)min((uint64_t)kWave, a.F - f0);
  float* __restrict__ blk = a.acc + f0 * C;
  const uint32_t nq = (uint32_t)kWave * C / 4u;   // float4 of a full block (64 * C floats: a multiple of four, 256-byte aligned)
  if (IN_LDS) {
    if (nrows == kWave) {
      const f4* b4 = reinterpret_cast<const f4*>(blk);
      for (uint32_t q0 = 0; q0 < nq; q0 += 4u * kWave) {
        f4 t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = b4[min(q0 + (uint32_t)j * kWave + (uint32_t)l, nq - 1u)];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t q = q0 + (uint32_t)j * kWave + (uint32_t)l;
          if (q < nq) {
            uint32_t r = q * 4u / C, c = q * 4u - r * C;
            const float e[4] = {t[j].x, t[j].y, t[j].z, t[j].w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
              srow[r * S + c] = e[k];
              if (++c == C) { c = 0u; r++; }
            }
          }
        }
      }
    } else {
      for (uint32_t q = l; q < (uint32_t)nrows * C; q += kWave) { const uint32_t r = q / C; srow[r * S + (q - r * C)] = blk[q]; }
    }
    wave_sync();
  }

  auto fuse_pixels = [&](auto* row) {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const unsigned long long m = msk[v];
      if (m == 0ull) continue;
      const uint32_t nv = (uint32_t)__popcll(m);   // this primitive's pixels in this view: the histogram entry of Mesh.h:90-93
      const float image_weight = 1.0f / ((float)nv);                           // Mesh.h:100
      const float pixel_w = 1.0f;                                              // :101
      const float w0 = a.iew * image_weight + (1 - a.iew) * pixel_w;           // :102
      const uint32_t x0 = org[v] & 0xFFFFu, y0 = org[v] >> 16, H = vw.v[v].H;
      const uint64_t last_run = (uint64_t)vw.v[v].W * H - 8u;   // (a run is clamped into the plane: the host refuses planes under 8 pixels)
      const LT* __restrict__ lab = static_cast<const LT*>(vw.v[v].labels);
      const float* __restrict__ wts = vw.v[v].weights;
      LabelRun<LT> run[8];
      uint32_t shift[8];
#pragma unroll
      for (int dx = 0; dx < 8; dx++) {
        shift[dx] = 0u;
        if ((m >> (dx * 8)) & 0xFFull) {
          const uint64_t s = (uint64_t)(x0 + (uint32_t)dx) * H + y0;
          const uint64_t sc = min(s, last_run);
          shift[dx] = (uint32_t)(s - sc);
          run[dx].load(lab + sc);
        }
      }
#pragma unroll
      for (int dx = 0; dx < 8; dx++) {
        uint32_t col = (uint32_t)(m >> (dx * 8)) & 0xFFu;
        while (col) {
          const uint32_t dy = (uint32_t)__ffs((int)col) - 1u;
          col &= col - 1u;
          const uint32_t c = run[dx].pick(dy + shift[dx]);
          const float wt = wts ? wts[(uint64_t)(x0 + (uint32_t)dx) * H + y0 + dy] : 1.0f;
          const float w = w0 * wt;                                             // :103
          if (c < C) row[c] = row[c] + 1.0f * w;
        }
      }
    }
  };
  if (IN_LDS) {
    fuse_pixels(srow + (uint32_t)l * S);
  } else {
    if (any_win) fuse_pixels(a.acc + f * C);   // (any_win: f < F and the triangle is nobody else's)
    return;
  }
  wave_sync();
  if (nrows != kWave || __ballot(big) != 0ull) {
    // some of these 64 rows belong to queued triangles, which the tail waves of this launch update meanwhile (or the block is the
    // mesh's last, partial one): every lane that added something stores its own row
    if (any_win) {
      float* __restrict__ mine = a.acc + f * C;
      for (uint32_t c = 0; c < C; c++) mine[c] = srow[(uint32_t)l * S + c];
    }
    return;
  }
  f4* b4 = reinterpret_cast<f4*>(blk);
  for (uint32_t q = l; q < nq; q += kWave) {
    uint32_t r = q * 4u / C, c = q * 4u - r * C;
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      e[k] = srow[r * S + c];
      if (++c == C) { c = 0u; r++; }
    }
    f4 t;
    t.x = e[0]; t.y = e[1]; t.z = e[2]; t.w = e[3];
    b4[q] = t;
  }
}

// Any accepted label image -> the dense (W,H) plane the fusion reads: every value outside [0, C) becomes the all-ones code.
template <typename T, typename OUT>
__global__ __launch_bounds__(256) void k_labels_narrow(const T* __restrict__ in, int64_t s0, int64_t s1, OUT* __restrict__ out, uint64_t N,
                                                       uint32_t H, uint32_t C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const uint64_t x = i / H, y = i - x * H;
  const T v = in[x * (uint64_t)s0 + y * (uint64_t)s1];
  bool ok = (uint64_t)v < (uint64_t)C;
  if (std::is_signed<T>::value) ok = ok && !(v < (T)0);
  out[i] = ok ? (OUT)v : (OUT)~(OUT)0;
}

// The fallback's expansion: a narrow label plane -> dense float32 (W,H,C) class vectors (tf.one_hot: all zero for a label >= C).
template <typename LT>
__global__ __launch_bounds__(256) void k_labels_onehot(const LT* __restrict__ lab, float* __restrict__ out, uint64_t total, uint32_t C) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint64_t i = e / C;
  out[e] = (uint32_t)lab[i] == (uint32_t)(e - i * C) ? 1.0f : 0.0f;
}

size_t label_itemsize(int dt) { return (size_t)1 << (dt >> 1); }

template <typename OUT>
void launch_narrow(const void* src, int dt, const int64_t s[2], OUT* out, uint64_t N, uint32_t H, uint32_t C, hipStream_t st) {
  const dim3 g((uint32_t)div_up(N, 256)), b(256);
  switch (dt) {
#define SMESH_NARROW(T) hipLaunchKernelGGL((k_labels_narrow<T, OUT>), g, b, 0, st, static_cast<const T*>(src), s[0], s[1], out, N, H, C); break
    case SMESH_LBL_U8:  SMESH_NARROW(uint8_t);
    case SMESH_LBL_I8:  SMESH_NARROW(int8_t);
    case SMESH_LBL_U16: SMESH_NARROW(uint16_t);
    case SMESH_LBL_I16: SMESH_NARROW(int16_t);
    case SMESH_LBL_U32: SMESH_NARROW(uint32_t);
    case SMESH_LBL_I32: SMESH_NARROW(int32_t);
    case SMESH_LBL_U64: SMESH_NARROW(uint64_t);
    default:            SMESH_NARROW(int64_t);
#undef SMESH_NARROW
  }
}

// (smesh_aggregator_create refuses more than 65535 classes; a uint16 plane -- 65535 = don't care -- could not name them all)
int check_label_classes(uint32_t C) {
  return C <= 65535u ? SMESH_OK : fail(SMESH_ERR_INVALID, "label images need an aggregator of at most 65535 classes");
}

int check_label_args(int dt, const int64_t s[2]) {
  if (dt < 0 || dt > SMESH_LBL_I64) return fail(SMESH_ERR_INVALID, "bad label dtype");
  if (s && (s[0] < 0 || s[1] < 0)) return fail(SMESH_ERR_INVALID, "labels: negative strides are not supported");
  return SMESH_OK;
}

// Is the image its own plane (a dense uint8 / uint16 image in device memory)?  Then narrow_plane needs no scratch for it.
bool plane_in_place(int dt, const int64_t* strides, int mem, uint64_t W, uint64_t H) {
  const bool is_dense = !strides || ((strides[0] == (int64_t)H || W == 1) && (strides[1] == 1 || H == 1));
  return mem == SMESH_MEM_DEVICE && (dt == SMESH_LBL_U8 || dt == SMESH_LBL_U16) && is_dense;
}

// The dense narrow plane of one label image, in device memory: the image itself where it is one already (dense uint8 / uint16 on the
// device: the kernels treat label >= C as don't-care), else slot `slot` of the plane scratch (`slot_bytes` apart), filled on the main
// stream -- a host image is staged first (*staged = true: the caller waits for the copies before it returns).
// `prep` (smesh_label_prep.h): the image is (prep->w, prep->h) and goes through `map_dev` (the call's map in device memory, or null):
// k_labels_prepare writes the plane -- always into the scratch, never in place --, a host image is staged at its own size and span.
int narrow_plane(DeviceCtx* ctx, LabelScratch& ls, int slot, size_t slot_bytes, size_t stage_bytes, const void* src, int dt, const int64_t* strides,
                 int mem, uint64_t W, uint64_t H, uint32_t C, const void** plane, int* label_bytes, bool* staged,
                 const LabelPrep* prep = nullptr, const LabelTableDev& table = LabelTableDev()) {
  const uint64_t N = W * H;
  if (prep) {
    const int ch = prep->channels;   // colour images (smesh_label_colors.h): three strides, uint8
    const int64_t own[3] = {(int64_t)prep->h * (ch ? ch : 1), ch ? ch : 1, 1};
    const int64_t* ps = strides ? strides : own;
    *label_bytes = C <= 255u ? 1 : 2;
    char* dst = static_cast<char*>(ls.plane.ptr) + (size_t)slot * slot_bytes;
    if (mem == SMESH_MEM_HOST) {
      *staged = true;
      const size_t span = (1 + (prep->w - 1) * (uint64_t)ps[0] + (prep->h - 1) * (uint64_t)ps[1] + (ch ? 2 * (uint64_t)ps[2] : 0)) * label_itemsize(dt);
      char* stage = static_cast<char*>(ls.stage.ptr) + (size_t)slot * stage_bytes;
      SMESH_HIP(hipMemcpyAsync(stage, src, span, hipMemcpyHostToDevice, ctx->stream));
      src = stage;
    }
    if (ch) SMESH_TRY(smesh_label_colors_launch(ctx, src, ps, prep->w, prep->h, table.keys, table.map, prep->table_len, C, dst, *label_bytes, W, H));
    else SMESH_TRY(smesh_label_prep_launch(ctx, src, dt, ps, prep->w, prep->h, table.map, prep->map_len, C, dst, *label_bytes, W, H));
    *plane = dst;
    return SMESH_OK;
  }
  const int64_t dense[2] = {(int64_t)H, 1};
  const int64_t* s = strides ? strides : dense;
  const bool is_dense = (s[0] == (int64_t)H || W == 1) && (s[1] == 1 || H == 1);
  const bool narrow = dt == SMESH_LBL_U8 || dt == SMESH_LBL_U16;
  const int out_bytes = narrow ? (int)label_itemsize(dt) : (C <= 255u ? 1 : 2);
  *label_bytes = out_bytes;
  if (mem == SMESH_MEM_DEVICE && narrow && is_dense) { *plane = src; return SMESH_OK; }   // (plane_in_place: no scratch was reserved)
  char* out = static_cast<char*>(ls.plane.ptr) + (size_t)slot * slot_bytes;
  if (mem == SMESH_MEM_HOST) {
    *staged = true;
    if (narrow && is_dense) {
      SMESH_HIP(hipMemcpyAsync(out, src, N * (size_t)out_bytes, hipMemcpyHostToDevice, ctx->stream));
      *plane = out;
      return SMESH_OK;
    }
    const size_t span = (1 + (W - 1) * (uint64_t)s[0] + (H - 1) * (uint64_t)s[1]) * label_itemsize(dt);
    char* stage = static_cast<char*>(ls.stage.ptr) + (size_t)slot * stage_bytes;
    SMESH_HIP(hipMemcpyAsync(stage, src, span, hipMemcpyHostToDevice, ctx->stream));
    src = stage;
  }
  if (out_bytes == 1) launch_narrow<uint8_t>(src, dt, s, reinterpret_cast<uint8_t*>(out), N, (uint32_t)H, C, ctx->stream);
  else launch_narrow<uint16_t>(src, dt, s, reinterpret_cast<uint16_t*>(out), N, (uint32_t)H, C, ctx->stream);
  SMESH_HIP(hipGetLastError());
  *plane = out;
  return SMESH_OK;
}

// (`channels`: a colour image of smesh_label_colors.h, three strides; its fourth channel is never read)
size_t stage_span_bytes(int dt, const int64_t* strides, uint64_t W, uint64_t H, int channels = 0) {
  const int64_t dense[3] = {(int64_t)H * (channels ? channels : 1), channels ? channels : 1, 1};
  const int64_t* s = strides ? strides : dense;
  return ((1 + (W - 1) * (uint64_t)s[0] + (H - 1) * (uint64_t)s[1] + (channels ? 2 * (uint64_t)s[2] : 0)) * label_itemsize(dt) + 255) & ~(size_t)255;
}

// The map of a prepared call in device memory: itself, or its copy in the aggregator's scratch (a host map: *staged = true).
// A colour table (always host memory) is staged as [keys][classes].
int stage_map(DeviceCtx* ctx, LabelScratch& ls, const LabelPrep* prep, LabelTableDev* table, bool* staged) {
  *table = LabelTableDev();
  if (prep && prep->channels) {
    const size_t kb = prep->table_len * 4;
    SMESH_TRY(ls.map.reserve(kb * 2));
    char* d = static_cast<char*>(ls.map.ptr);
    SMESH_HIP(hipMemcpyAsync(d, prep->keys, kb, hipMemcpyHostToDevice, ctx->stream));
    SMESH_HIP(hipMemcpyAsync(d + kb, prep->classes, kb, hipMemcpyHostToDevice, ctx->stream));
    table->keys = reinterpret_cast<const uint32_t*>(d);
    table->map = reinterpret_cast<const int32_t*>(d + kb);
    *staged = true;
    return SMESH_OK;
  }
  if (!prep || !prep->map) return SMESH_OK;
  if (prep->map_mem == SMESH_MEM_DEVICE) { table->map = prep->map; return SMESH_OK; }
  SMESH_TRY(ls.map.reserve(prep->map_len * 4));
  SMESH_HIP(hipMemcpyAsync(ls.map.ptr, prep->map, prep->map_len * 4, hipMemcpyHostToDevice, ctx->stream));
  table->map = static_cast<const int32_t*>(ls.map.ptr);
  *staged = true;
  return SMESH_OK;
}

}  // namespace

// ---- what raster.hip calls --------------------------------------------------------------------------------------------------

// Do label views of an image of N pixels, rendered by a triangle renderer of F triangles in the caller's face order, take
// k_fuse_tri_labels for this aggregator?  Sum / Summax only (Mul is defined on one-hot input -- log 0 = -inf for every class but one --
// and takes the class-vector path), rows in triangle order, a plane of at least one run of eight labels.
bool smesh_labels_native(smesh_aggregator* a, uint64_t F, uint64_t N) {
  int kind;
  smesh_aggregator_label_target(a, nullptr, nullptr, nullptr, &kind, nullptr);
  return kind != SMESH_AGG_MUL && F != 0 && N >= 8 && smesh_aggregator_can_fuse_triangles(a, F);
}

// Reporting only (the read-only option "last_fuse_labels_form"): the instance of the calling thread's last k_fuse_tri_labels launch
// beyond its view count -- bytes per label of the planes (1 or 2), plus 16 where the rows were kept in LDS; 0 before the first launch.
static thread_local int g_last_labels_form = 0;
int smesh_last_labels_form() { return g_last_labels_form; }

// views[v].image: dense narrow planes of `label_bytes` (1 or 2) bytes per pixel in device memory.  `nviews` = 1, 2, 4 or 8.
int smesh_labels_fuse_triangles(smesh_aggregator* a, uint64_t F, uint32_t big_capacity, const RenderedView* views, int nviews, int label_bytes) {
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  hipStream_t st = ctx->stream;
  if (F == 0) return SMESH_OK;
  LabelFuseArgs t;
  int kind;
  SMESH_TRY(check_fuse_rows("fuse_triangles_labels", "fuse_view_labels()", a, F, nviews, 0, &t, &kind));
  if (label_bytes != 1 && label_bytes != 2) return fail(SMESH_ERR_INVALID, "fuse_triangles_labels: label planes are uint8 or uint16");
  LabelViews<8> tv;
  for (int v = 0; v < 8; v++) {
    const RenderedView& rv = views[v < nviews ? v : 0];
    if (rv.W * rv.H < 8 || !rv.image) return fail(SMESH_ERR_INVALID, "fuse_triangles_labels: label plane missing or under 8 pixels");
    tv.v[v] = LabelView{rv.frags, rv.idx, rv.image, rv.weights, rv.big_queue, rv.big_len, (uint32_t)rv.W, (uint32_t)rv.H};
  }
  const bool in_lds = t.C <= kLabelsLdsMaxC;
  const dim3 grid = fuse_rows_grid(ctx, F, big_capacity, views, nviews, &t), block(kWave);
  t.stride = t.C | 1u;
  const size_t lds = in_lds ? (size_t)kWave * t.stride * 4 : 0;
  ProfScope prof(ctx, SMESH_PROF_FUSE_SCATTER);
  prof_note(ctx, SMESH_PROF_FUSE_SCATTER, 1, (uint64_t)nviews);
  auto launch = [&](auto lt, auto NV) {   // (one kind, no class slots: the class count is a run-time value, the row an LDS block or memory)
    using LT = decltype(lt);
    if (in_lds) hipLaunchKernelGGL((k_fuse_tri_labels<LT, NV(), true>), grid, block, lds, st, t, (first_views<LabelViews, NV()>(tv)));
    else hipLaunchKernelGGL((k_fuse_tri_labels<LT, NV(), false>), grid, block, 0, st, t, (first_views<LabelViews, NV()>(tv)));
  };
  launch_fuse_rows<false>(0, kind, nviews, [&](auto, auto, auto NV) {
    if (label_bytes == 1) launch(uint8_t(), NV);
    else launch(uint16_t(), NV);
  });
  g_last_labels_form = label_bytes + (in_lds ? 16 : 0);
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// The fallback's class vectors: one_hot of a narrow device plane as dense float32 (W,H,C) in the aggregator's label scratch, on the
// main stream.  One buffer: whoever reads it is queued on that stream before the next expansion.
int smesh_labels_expand(smesh_aggregator* a, const void* plane, int label_bytes, uint64_t N, const float** probs) {
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  LabelScratch& ls = smesh_aggregator_label_scratch(a);
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  const uint64_t total = N * C;
  SMESH_TRY(ls.onehot.reserve(std::max<uint64_t>(total * 4, 16)));
  float* out = static_cast<float*>(ls.onehot.ptr);
  if (total) {
    const dim3 g((uint32_t)div_up(total, 256)), b(256);
    if (label_bytes == 1) hipLaunchKernelGGL(k_labels_onehot<uint8_t>, g, b, 0, ctx->stream, static_cast<const uint8_t*>(plane), out, total, C);
    else hipLaunchKernelGGL(k_labels_onehot<uint16_t>, g, b, 0, ctx->stream, static_cast<const uint16_t*>(plane), out, total, C);
    SMESH_HIP(hipGetLastError());
  }
  *probs = out;
  return SMESH_OK;
}

// ---- the entry points, with and without preparation ------------------------------------------------------------------------------
// `prep` null: smesh_labels.h; else smesh_label_prep.h -- the same call from narrow_plane() on.
static int fuse_views_labels_impl(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* labels,
                                  int label_dtype, const int64_t label_strides[2], const float* const* weights, int memkind,
                                  const LabelPrep* prep) {
  if (!r || !a || (n && (!cams || !labels))) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(check_label_args(label_dtype, label_strides));
  if (memkind != SMESH_MEM_HOST && memkind != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (prep && prep->channels) SMESH_TRY(smesh_label_colors_check(label_dtype, label_strides, *prep));
  for (uint64_t i = 0; i < n; i++) {
    if (!labels[i]) return fail(SMESH_ERR_INVALID, "NULL label image");
    if (cams[i].width == 0 || cams[i].height == 0 || cams[i].width > 65536 || cams[i].height > 65536)
      return fail(SMESH_ERR_INVALID, "camera resolution must be in [1, 65536]");
  }
  DeviceCtx* ctx = smesh_renderer_ctx(r);
  if (smesh_aggregator_ctx(a) != ctx) return fail(SMESH_ERR_INVALID, "renderer and aggregator live on different devices");
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  SMESH_TRY(check_label_classes(C));
  if (prep) {
    for (uint64_t i = 0; i < n; i++) SMESH_TRY(smesh_label_prep_check(label_dtype, label_strides, memkind, *prep, cams[i].width, cams[i].height, C));
  }
  LabelTableDev table;
  bool map_staged = false;
  LabelScratch& ls = smesh_aggregator_label_scratch(a);
  std::lock_guard<std::mutex> g(ls.mu);
  // groups of up to eight views: their planes (and staged host images and weights) share the scratch, which the next group's copies
  // and narrowing kernels overwrite behind this group's fusion on the main stream
  for (uint64_t i = 0; i < n; i += kGroup) {
    const int m = (int)std::min<uint64_t>(kGroup, n - i);
    size_t slot_bytes = 0, stage_bytes = 0, w_bytes = 0;
    for (int v = 0; v < m; v++) {
      const uint64_t N = cams[i + v].width * cams[i + v].height;
      slot_bytes = std::max(slot_bytes, round256(N * 2));
      stage_bytes = std::max(stage_bytes, prep ? stage_span_bytes(label_dtype, label_strides, prep->w, prep->h, prep->channels)
                                                  : stage_span_bytes(label_dtype, label_strides, cams[i + v].width, cams[i + v].height));
      w_bytes = std::max(w_bytes, round256(N * 4));
    }
    const void* planes[kGroup];
    const float* wts[kGroup];
    int label_bytes = 1;
    bool staged = false;
    {
      std::lock_guard<std::recursive_mutex> lock(ctx->mu);
      SMESH_HIP(hipSetDevice(ctx->device));
      if (i == 0) {
        SMESH_TRY(stage_map(ctx, ls, prep, &table, &map_staged));
        staged = map_staged;
      }
      bool in_place = !prep;   // nothing to narrow: no plane scratch (a prepared plane is always scratch)
      for (int v = 0; v < m; v++) in_place = in_place && plane_in_place(label_dtype, label_strides, memkind, cams[i + v].width, cams[i + v].height);
      if (!in_place) SMESH_TRY(ls.plane.reserve(slot_bytes * (size_t)m));
      if (memkind == SMESH_MEM_HOST) {
        SMESH_TRY(ls.stage.reserve(stage_bytes * (size_t)m));
        if (weights) SMESH_TRY(ls.w.reserve(w_bytes * (size_t)m));
      }
      for (int v = 0; v < m; v++) {
        const uint64_t W = cams[i + v].width, H = cams[i + v].height;
        SMESH_TRY(narrow_plane(ctx, ls, v, slot_bytes, stage_bytes, labels[i + v], label_dtype, label_strides, memkind, W, H, C, &planes[v],
                               &label_bytes, &staged, prep, table));
        wts[v] = weights ? weights[i + v] : nullptr;
        if (wts[v] && memkind == SMESH_MEM_HOST) {
          float* d = reinterpret_cast<float*>(static_cast<char*>(ls.w.ptr) + (size_t)v * w_bytes);
          SMESH_HIP(hipMemcpyAsync(d, wts[v], W * H * 4, hipMemcpyHostToDevice, ctx->stream));
          wts[v] = d;
          staged = true;
        }
      }
      if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // the caller may reuse its host arrays once we return
    }
    SMESH_TRY(smesh_renderer_fuse_views_labels(r, a, &cams[i], (uint64_t)m, planes, weights ? wts : nullptr, ViewInput::labels(nullptr, label_bytes)));
  }
  return SMESH_OK;
}

static int add_labels_impl(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                           int idx_mem, const void* labels, int label_dtype, const int64_t label_strides[2], int label_mem,
                           const float* weights, const int64_t w_strides[2], int w_mem, uint64_t W, uint64_t H, const LabelPrep* prep) {
  if (!a || !indices || !labels) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (idx_dtype < 0 || idx_dtype > 3) return fail(SMESH_ERR_INVALID, "bad index dtype");
  SMESH_TRY(check_label_args(label_dtype, label_strides));
  if ((idx_strides && (idx_strides[0] < 0 || idx_strides[1] < 0)) || (weights && w_strides && (w_strides[0] < 0 || w_strides[1] < 0)))
    return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  uint32_t C;
  smesh_aggregator_label_target(a, nullptr, nullptr, &C, nullptr, nullptr);
  if (prep) {
    if (label_mem != SMESH_MEM_HOST && label_mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
    if (prep->channels) SMESH_TRY(smesh_label_colors_check(label_dtype, label_strides, *prep));
    SMESH_TRY(smesh_label_prep_check(label_dtype, label_strides, label_mem, *prep, W, H, C));
  }
  if (W == 0 || H == 0) return SMESH_OK;
  if (W > 65536 || H > 65536 || W * H >= 0x7FFFFFFFull / 4) return fail(SMESH_ERR_INVALID, "image too large");
  DeviceCtx* ctx = smesh_aggregator_ctx(a);
  if (r && smesh_renderer_ctx(r) != ctx) r = nullptr;
  const uint64_t N = W * H;
  const int64_t dense[2] = {(int64_t)H, 1};
  const int64_t* is = idx_strides ? idx_strides : dense;
  const int64_t* ws = w_strides ? w_strides : dense;
  SMESH_TRY(check_label_classes(C));
  LabelScratch& ls = smesh_aggregator_label_scratch(a);
  std::lock_guard<std::mutex> g(ls.mu);
  const void* plane = nullptr;
  const float* d_w = weights;
  int label_bytes = 1;
  bool staged = false;
  const bool w_dense = !weights || (ws[0] == (int64_t)H && ws[1] == 1);
  const bool rendered = r && idx_mem == SMESH_MEM_DEVICE && idx_dtype == SMESH_IDX_U32 && is[0] == (int64_t)H && is[1] == 1 && w_dense;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    LabelTableDev table;
    SMESH_TRY(stage_map(ctx, ls, prep, &table, &staged));
    if (prep || !plane_in_place(label_dtype, label_strides, label_mem, W, H)) SMESH_TRY(ls.plane.reserve(round256(N * 2)));
    if (label_mem == SMESH_MEM_HOST)
      SMESH_TRY(ls.stage.reserve(prep ? stage_span_bytes(label_dtype, label_strides, prep->w, prep->h, prep->channels) : stage_span_bytes(label_dtype, label_strides, W, H)));
    SMESH_TRY(narrow_plane(ctx, ls, 0, round256(N * 2), 0, labels, label_dtype, label_strides, label_mem, W, H, C, &plane, &label_bytes, &staged,
                           prep, table));
    if (rendered && weights && w_mem == SMESH_MEM_HOST) {   // (the triangle-order kernel wants the weights where the plane is)
      SMESH_TRY(ls.w.reserve(N * 4));
      SMESH_HIP(hipMemcpyAsync(ls.w.ptr, weights, N * 4, hipMemcpyHostToDevice, ctx->stream));
      d_w = static_cast<const float*>(ls.w.ptr);
      staged = true;
    }
    if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host images are consumed before the call returns
  }
  if (rendered) {
    int done = 0;
    SMESH_TRY(smesh_renderer_add_rendered_input(a, r, static_cast<const uint32_t*>(indices), ViewInput::labels(plane, label_bytes), d_w, W, H, &done));
    if (done) return SMESH_OK;
  }
  // everything else: the labels expanded on the device, then the class-vector path unchanged (asynchronous for device images)
  const float* probs = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    SMESH_HIP(hipSetDevice(ctx->device));
    SMESH_TRY(smesh_labels_expand(a, plane, label_bytes, N, &probs));
  }
  const int64_t ps[3] = {(int64_t)(H * C), (int64_t)C, 1};
  return smesh_aggregator_add_async(a, indices, idx_dtype, is, idx_mem, probs, ps, SMESH_MEM_DEVICE, weights, ws, w_mem, W, H);
}

// ---- include/smesh_labels.h, include/smesh_label_prep.h, include/smesh_label_colors.h -----------------------------------------------
static LabelPrep color_prep(uint64_t w, uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K) {
  LabelPrep p{w, h, nullptr, 0, SMESH_MEM_HOST};
  p.channels = channels ? channels : -1;   // (0 is "no colour image" inside: a refused count either way)
  p.keys = keys; p.classes = classes; p.table_len = K;
  return p;
}

extern "C" {

int smesh_fuse_views_labels(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* labels,
                            int label_dtype, const int64_t label_strides[2], const float* const* weights, int memkind) {
  return fuse_views_labels_impl(r, a, cams, n, labels, label_dtype, label_strides, weights, memkind, nullptr);
}

int smesh_fuse_view_labels(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cam, const void* labels, int label_dtype,
                           const int64_t label_strides[2], const float* weights, int memkind) {
  if (!cam) return fail(SMESH_ERR_INVALID, "NULL argument");
  return fuse_views_labels_impl(r, a, cam, 1, &labels, label_dtype, label_strides, weights ? &weights : nullptr, memkind, nullptr);
}

int smesh_aggregator_add_labels(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                int idx_mem, const void* labels, int label_dtype, const int64_t label_strides[2], int label_mem,
                                const float* weights, const int64_t w_strides[2], int w_mem, uint64_t W, uint64_t H) {
  return add_labels_impl(a, r, indices, idx_dtype, idx_strides, idx_mem, labels, label_dtype, label_strides, label_mem, weights, w_strides, w_mem, W, H,
                         nullptr);
}

int smesh_fuse_views_labels_prepared(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* labels,
                                     int label_dtype, const int64_t label_strides[2], const float* const* weights, int memkind, uint64_t w,
                                     uint64_t h, const int32_t* map, uint64_t map_len, int map_memkind) {
  const LabelPrep prep{w, h, map, map_len, map_memkind};
  return fuse_views_labels_impl(r, a, cams, n, labels, label_dtype, label_strides, weights, memkind, &prep);
}

int smesh_fuse_view_labels_prepared(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cam, const void* labels, int label_dtype,
                                    const int64_t label_strides[2], const float* weights, int memkind, uint64_t w, uint64_t h,
                                    const int32_t* map, uint64_t map_len, int map_memkind) {
  if (!cam) return fail(SMESH_ERR_INVALID, "NULL argument");
  const LabelPrep prep{w, h, map, map_len, map_memkind};
  return fuse_views_labels_impl(r, a, cam, 1, &labels, label_dtype, label_strides, weights ? &weights : nullptr, memkind, &prep);
}

int smesh_aggregator_add_labels_prepared(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype,
                                         const int64_t idx_strides[2], int idx_mem, const void* labels, int label_dtype,
                                         const int64_t label_strides[2], int label_mem, const float* weights, const int64_t w_strides[2],
                                         int w_mem, uint64_t W, uint64_t H, uint64_t w, uint64_t h, const int32_t* map, uint64_t map_len,
                                         int map_memkind) {
  const LabelPrep prep{w, h, map, map_len, map_memkind};
  return add_labels_impl(a, r, indices, idx_dtype, idx_strides, idx_mem, labels, label_dtype, label_strides, label_mem, weights, w_strides, w_mem, W, H,
                         &prep);
}

int smesh_fuse_views_labels_colors(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, uint64_t n, const void* const* labels,
                                   int label_dtype, const int64_t label_strides[3], const float* const* weights, int memkind, uint64_t w,
                                   uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K) {
  const LabelPrep prep = color_prep(w, h, channels, keys, classes, K);
  return fuse_views_labels_impl(r, a, cams, n, labels, label_dtype, label_strides, weights, memkind, &prep);
}

int smesh_fuse_view_labels_colors(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cam, const void* labels, int label_dtype,
                                  const int64_t label_strides[3], const float* weights, int memkind, uint64_t w, uint64_t h, int channels,
                                  const uint32_t* keys, const int32_t* classes, uint64_t K) {
  if (!cam) return fail(SMESH_ERR_INVALID, "NULL argument");
  const LabelPrep prep = color_prep(w, h, channels, keys, classes, K);
  return fuse_views_labels_impl(r, a, cam, 1, &labels, label_dtype, label_strides, weights ? &weights : nullptr, memkind, &prep);
}

int smesh_aggregator_add_labels_colors(smesh_aggregator_t* a, smesh_renderer_t* r, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                       int idx_mem, const void* labels, int label_dtype, const int64_t label_strides[3], int label_mem,
                                       const float* weights, const int64_t w_strides[2], int w_mem, uint64_t W, uint64_t H, uint64_t w,
                                       uint64_t h, int channels, const uint32_t* keys, const int32_t* classes, uint64_t K) {
  const LabelPrep prep = color_prep(w, h, channels, keys, classes, K);
  return add_labels_impl(a, r, indices, idx_dtype, idx_strides, idx_mem, labels, label_dtype, label_strides, label_mem, weights, w_strides, w_mem, W, H,
                         &prep);
}

}  // extern "C"
