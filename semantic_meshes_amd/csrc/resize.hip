// resize.hip -- class-vector images resampled from the network's resolution to the camera's (include/smesh_resize.h): the dense
// (W,H,C) image the fusion kernels read, the labels of that image without building it, and those labels counted against ground truth.
//
// Reference: eval-scannet/eval_scannet.py:221-236 (the (480,640,40) prediction resized to (968,1296,40) by tf.image.resize before
// it is scored and fused), python/scripts/colorize_cityscapes_mesh.py:42 (multi_scale(predictor, [0.5])).
//
// The rule is evaluated in ONE place, axis_of() and blend() of resize_rule.hpp: the source coordinates in double, the three lerps
// in float32, every operation rounded separately (the library is built with -ffp-contract=off).  No result depends on the path, the
// dtype pair's load width or the launch shape.
#include "confusion.hpp"
#include "half_scratch.hpp"
#include "resize_rule.hpp"

#include <cmath>

#include "../../include/smesh_resize.h"

using namespace smesh;

namespace {

constexpr int kRsBlock = 256;
constexpr uint32_t kMaxGridY = 65535;

size_t probs_itemsize(int dt) { return dt == SMESH_PROBS_F32 ? 4 : 2; }
bool bad_probs_dtype(int dt) { return dt != SMESH_PROBS_F32 && dt != SMESH_PROBS_F16 && dt != SMESH_PROBS_BF16; }

typedef uint32_t rs_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rs_u32x2 __attribute__((ext_vector_type(2)));

struct RsArgs {
  const void* in;
  int64_t s0, s1, s2;           // element strides of x, y and the class of `in`
  double sx, sy;                // (double)w / (double)W and (double)h / (double)H, divided on the host
  uint32_t w, h, W, H, C;
  int in_dtype;
  // smesh_resize_probs
  void* out;                    // dense (W,H,C) of out_dtype
  int out_dtype;
  uint32_t CV;                  // vector path: 16-byte pieces of a pixel's row
  uint64_t col;                 // work items of one output column: H CV pieces, or H C elements
  // smesh_resize_probs_labels
  void* lbl;                    // label image of `lbl_dtype` (SMESH_LBL_U8 / _U16 / _I32), or null
  int64_t os0, os1;
  int32_t* lbl32;               // dense int32 (W,H), y fastest, -1 for don't care (what k_confusion counts), or null
  int lbl_dtype;
  uint32_t dc_value;
  float thr;
  int use_sum;
};

// (Axis, axis_of(), lerp1() and blend(): resize_rule.hpp, shared with fusion_sampled.hip)

__device__ __forceinline__ float load_elem(const void* p, int dt, uint64_t off) {
  if (dt == SMESH_PROBS_F32) return static_cast<const float*>(p)[off];
  float lo, hi;
  unpack2((uint32_t) static_cast<const uint16_t*>(p)[off], dt == SMESH_PROBS_BF16, lo, hi);
  return lo;
}
__device__ __forceinline__ uint32_t narrow1(float v, bool bf) { return bf ? bf16_rne(v) : f16_rne(v); }

// VE consecutive elements of EB bytes each at `p` (aligned to min(VE EB, 16) bytes), widened.
template <int EB, int VE>
__device__ __forceinline__ void load_row(const char* p, bool bf, float (&v)[VE]) {
  if constexpr (EB == 4) {
#pragma unroll
    for (int k = 0; k < VE; k += 4) {
      const rs_u32x4 q = *reinterpret_cast<const rs_u32x4*>(p + k * 4);
      v[k] = __uint_as_float(q.x); v[k + 1] = __uint_as_float(q.y); v[k + 2] = __uint_as_float(q.z); v[k + 3] = __uint_as_float(q.w);
    }
  } else if constexpr (VE == 8) {
    const rs_u32x4 q = *reinterpret_cast<const rs_u32x4*>(p);
    unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]); unpack2(q.z, bf, v[4], v[5]); unpack2(q.w, bf, v[6], v[7]);
  } else {
    const rs_u32x2 q = *reinterpret_cast<const rs_u32x2*>(p);
    unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]);
  }
}

// VECTOR path: a lane owns 16 bytes of the dense output -- VE = 16 / OEB classes of one pixel -- and lanes run along the output's
// memory order inside a column (y, then the class), so a wave's stores are 1 KiB contiguous.  blockIdx.y is the column: no 64-bit
// division, and the x axis is the same for the whole workgroup.  Four corner loads of VE IEB bytes (8, 16 or 2 x 16), which L2 and
// the Infinity Cache serve (the source is about a quarter of the output, and neighbouring lanes share corners): no LDS staging.
template <int IEB, int OEB>
__global__ __launch_bounds__(kRsBlock) void k_resize_probs(RsArgs a) {
  constexpr int VE = 16 / OEB;
  const uint32_t v = blockIdx.x * kRsBlock + threadIdx.x;
  if (v >= (uint32_t)a.col) return;
  const uint32_t Y = v / a.CV, c = (v - Y * a.CV) * VE;
  const Axis ay = axis_of(Y, a.sy, a.h);
  const bool ibf = a.in_dtype == SMESH_PROBS_BF16, obf = a.out_dtype == SMESH_PROBS_BF16;
  const char* in = static_cast<const char*>(a.in);
  const uint64_t r0 = (uint64_t)ay.i0 * (uint64_t)a.s1 + c, r1 = (uint64_t)ay.i1 * (uint64_t)a.s1 + c;
  for (uint32_t X = blockIdx.y; X < a.W; X += gridDim.y) {
    const Axis ax = axis_of(X, a.sx, a.w);
    const uint64_t c0 = (uint64_t)ax.i0 * (uint64_t)a.s0, c1 = (uint64_t)ax.i1 * (uint64_t)a.s0;
    float a00[VE], a10[VE], a01[VE], a11[VE];
    load_row<IEB, VE>(in + (c0 + r0) * IEB, ibf, a00);
    load_row<IEB, VE>(in + (c1 + r0) * IEB, ibf, a10);
    load_row<IEB, VE>(in + (c0 + r1) * IEB, ibf, a01);
    load_row<IEB, VE>(in + (c1 + r1) * IEB, ibf, a11);
    float r[VE];
#pragma unroll
    for (int k = 0; k < VE; k++) r[k] = blend(a00[k], a10[k], a01[k], a11[k], ax.f, ay.f);
    const uint64_t o = ((uint64_t)X * a.H + Y) * a.C + c;
    rs_u32x4 q;
    if constexpr (OEB == 4) {
      q.x = __float_as_uint(r[0]); q.y = __float_as_uint(r[1]); q.z = __float_as_uint(r[2]); q.w = __float_as_uint(r[3]);
    } else {
      q.x = narrow1(r[0], obf) | (narrow1(r[1], obf) << 16); q.y = narrow1(r[2], obf) | (narrow1(r[3], obf) << 16);
      q.z = narrow1(r[4], obf) | (narrow1(r[5], obf) << 16); q.w = narrow1(r[6], obf) | (narrow1(r[7], obf) << 16);
    }
    *reinterpret_cast<rs_u32x4*>(static_cast<char*>(a.out) + o * OEB) = q;
  }
}

// GENERIC path: any strides, class count and alignment.  One lane per output element, the same column-per-blockIdx.y shape.
// Correct, not fast.
__global__ __launch_bounds__(kRsBlock) void k_resize_probs_generic(RsArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kRsBlock + threadIdx.x;
  if (e >= a.col) return;
  const uint32_t Y = (uint32_t)(e / a.C), c = (uint32_t)(e - (uint64_t)Y * a.C);
  const Axis ay = axis_of(Y, a.sy, a.h);
  const uint64_t r0 = (uint64_t)ay.i0 * (uint64_t)a.s1 + (uint64_t)c * (uint64_t)a.s2;
  const uint64_t r1 = (uint64_t)ay.i1 * (uint64_t)a.s1 + (uint64_t)c * (uint64_t)a.s2;
  for (uint32_t X = blockIdx.y; X < a.W; X += gridDim.y) {
    const Axis ax = axis_of(X, a.sx, a.w);
    const uint64_t c0 = (uint64_t)ax.i0 * (uint64_t)a.s0, c1 = (uint64_t)ax.i1 * (uint64_t)a.s0;
    const float r = blend(load_elem(a.in, a.in_dtype, c0 + r0), load_elem(a.in, a.in_dtype, c1 + r0),
                          load_elem(a.in, a.in_dtype, c0 + r1), load_elem(a.in, a.in_dtype, c1 + r1), ax.f, ay.f);
    const uint64_t o = (uint64_t)X * a.col + e;
    if (a.out_dtype == SMESH_PROBS_F32) static_cast<float*>(a.out)[o] = r;
    else static_cast<uint16_t*>(a.out)[o] = (uint16_t)narrow1(r, a.out_dtype == SMESH_PROBS_BF16);
  }
}

// The running state of one pixel's scan: the rule of smesh_probs_labels.h, classes in ascending order.
struct Scan {
  float best, sum;
  uint32_t label;
  __device__ __forceinline__ void take(uint32_t c, float v, int use_sum) {
    if (use_sum) sum += v;
    if (c == 0u) best = v;
    else if (v > best) { best = v; label = c; }
  }
};

// Labels of the resampled image: one lane per output pixel (blockIdx.y: the column, lanes along y), classes in ascending order, each
// blended and scanned as it comes; no (W,H,C) image anywhere.  VEC: class stride 1 with aligned rows -- the classes come in 16-byte
// pieces per corner, the last C % VE one by one.  EB: bytes per element.
template <int EB, bool VEC>
__global__ __launch_bounds__(kRsBlock) void k_resize_probs_labels(RsArgs a) {
  constexpr int VE = 16 / EB;
  const uint32_t Y = blockIdx.x * kRsBlock + threadIdx.x;
  if (Y >= a.H) return;
  const Axis ay = axis_of(Y, a.sy, a.h);
  const bool bf = a.in_dtype == SMESH_PROBS_BF16;
  const uint32_t C = a.C;
  const uint64_t r0 = (uint64_t)ay.i0 * (uint64_t)a.s1, r1 = (uint64_t)ay.i1 * (uint64_t)a.s1;
  for (uint32_t X = blockIdx.y; X < a.W; X += gridDim.y) {
    const Axis ax = axis_of(X, a.sx, a.w);
    const uint64_t c0 = (uint64_t)ax.i0 * (uint64_t)a.s0, c1 = (uint64_t)ax.i1 * (uint64_t)a.s0;
    const uint64_t p00 = c0 + r0, p10 = c1 + r0, p01 = c0 + r1, p11 = c1 + r1;
    Scan s;
    s.best = 0.0f; s.sum = 0.0f; s.label = 0u;
    uint32_t c = 0;
    if constexpr (VEC) {
      const char* in = static_cast<const char*>(a.in);
      for (; c + VE <= C; c += VE) {
        float a00[VE], a10[VE], a01[VE], a11[VE];
        load_row<EB, VE>(in + (p00 + c) * EB, bf, a00);
        load_row<EB, VE>(in + (p10 + c) * EB, bf, a10);
        load_row<EB, VE>(in + (p01 + c) * EB, bf, a01);
        load_row<EB, VE>(in + (p11 + c) * EB, bf, a11);
#pragma unroll
        for (int k = 0; k < VE; k++) s.take(c + k, blend(a00[k], a10[k], a01[k], a11[k], ax.f, ay.f), a.use_sum);
      }
    }
    for (; c < C; c++) {
      const uint64_t k = (uint64_t)c * (uint64_t)a.s2;
      s.take(c, blend(load_elem(a.in, a.in_dtype, p00 + k), load_elem(a.in, a.in_dtype, p10 + k),
                      load_elem(a.in, a.in_dtype, p01 + k), load_elem(a.in, a.in_dtype, p11 + k), ax.f, ay.f), a.use_sum);
    }
    const bool dc = a.use_sum && s.sum < a.thr;
    if (a.lbl) {
      const uint64_t o = (uint64_t)X * (uint64_t)a.os0 + (uint64_t)Y * (uint64_t)a.os1;
      const uint32_t v = dc ? a.dc_value : s.label;
      if (a.lbl_dtype == SMESH_LBL_U8) static_cast<uint8_t*>(a.lbl)[o] = (uint8_t)v;
      else if (a.lbl_dtype == SMESH_LBL_U16) static_cast<uint16_t*>(a.lbl)[o] = (uint16_t)v;
      else static_cast<uint32_t*>(a.lbl)[o] = v;
    }
    if (a.lbl32) a.lbl32[(uint64_t)X * a.H + Y] = dc ? -1 : (int32_t)s.label;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// The checks all three entry points share; fills the source and geometry part of `a`.  W and H are not zero.
int check_source(RsArgs& a, const char* who, const void* in, int dt, const int64_t* s, int mem, uint64_t w, uint64_t h, uint32_t C,
                 uint64_t W, uint64_t H, int mode) {
  const std::string p = std::string(who) + ": ";
  if (!in) return fail(SMESH_ERR_INVALID, p + "NULL class-vector image");
  if (bad_probs_dtype(dt)) return fail(SMESH_ERR_INVALID, p + "bad class-vector dtype");
  if (mode != SMESH_RESIZE_BILINEAR) return fail(SMESH_ERR_INVALID, p + "unknown resampling mode");
  if (s && (s[0] < 0 || s[1] < 0 || s[2] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (bad_mem(mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (reinterpret_cast<uintptr_t>(in) % probs_itemsize(dt)) return fail(SMESH_ERR_INVALID, p + "the image is not aligned to its element size");
  if (C == 0) return fail(SMESH_ERR_INVALID, p + "the class count must be positive");
  if (w == 0 || h == 0) return fail(SMESH_ERR_INVALID, p + "an empty source image cannot fill a non-empty target");
  SMESH_TRY(check_image_size(W, H));
  if (w > 65536 || h > 65536) return fail(SMESH_ERR_INVALID, "image too large");
  a.in = in;
  a.in_dtype = dt;
  a.s0 = s ? s[0] : (int64_t)(h * C);
  a.s1 = s ? s[1] : (int64_t)C;
  a.s2 = s ? s[2] : 1;
  a.w = (uint32_t)w; a.h = (uint32_t)h; a.W = (uint32_t)W; a.H = (uint32_t)H; a.C = C;
  a.sx = (double)w / (double)W;
  a.sy = (double)h / (double)H;
  return SMESH_OK;
}

// Elements that the strides of the source cover.
uint64_t source_span(const RsArgs& a) {
  return 1 + (uint64_t)(a.w - 1) * (uint64_t)a.s0 + (uint64_t)(a.h - 1) * (uint64_t)a.s1 + (uint64_t)(a.C - 1) * (uint64_t)a.s2;
}

int check_no_overlap(const char* who, const RsArgs& a, const void* out, uint64_t out_bytes) {
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(a.in), i1 = i0 + source_span(a) * probs_itemsize(a.in_dtype);
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + out_bytes;
  if (o0 < i1 && i0 < o1) return fail(SMESH_ERR_INVALID, std::string(who) + ": the output overlaps the input");
  return SMESH_OK;
}

int check_labels_out(RsArgs& a, const char* who, int out_dtype, const int64_t* os, int64_t dcv, uint64_t H, uint32_t C, float thr) {
  const std::string p = std::string(who) + ": ";
  if (thr != thr) return fail(SMESH_ERR_INVALID, p + "the don't-care threshold is NaN");
  a.thr = thr;
  a.use_sum = (std::isinf(thr) && thr < 0) ? 0 : 1;
  if (!a.lbl) return SMESH_OK;
  if (out_dtype != SMESH_LBL_U8 && out_dtype != SMESH_LBL_U16 && out_dtype != SMESH_LBL_I32)
    return fail(SMESH_ERR_INVALID, p + "the label image must be uint8, uint16 or int32");
  if (os && (os[0] < 0 || os[1] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  const int64_t lo = out_dtype == SMESH_LBL_I32 ? -2147483648ll : 0;
  const int64_t hi = out_dtype == SMESH_LBL_U8 ? 255 : out_dtype == SMESH_LBL_U16 ? 65535 : 2147483647ll;
  if ((int64_t)C - 1 > hi || (out_dtype != SMESH_LBL_I32 && (int64_t)C > hi))
    return fail(SMESH_ERR_INVALID, p + "the label dtype is too narrow for the class count");
  if (dcv < lo || dcv > hi) return fail(SMESH_ERR_INVALID, p + "the label dtype cannot hold the don't-care value");
  if (dcv >= 0 && dcv < (int64_t)C) return fail(SMESH_ERR_INVALID, p + "the don't-care value is a class");
  a.lbl_dtype = out_dtype;
  a.os0 = os ? os[0] : (int64_t)H;
  a.os1 = os ? os[1] : 1;
  a.dc_value = (uint32_t)(int32_t)dcv;
  return SMESH_OK;
}

// A HOST source staged at its own size and width: the span its strides cover.
int source_on_device(DeviceCtx* ctx, Scratch& stage, RsArgs& a, int mem, bool* staged) {
  if (mem == SMESH_MEM_DEVICE) return SMESH_OK;
  const size_t bytes = (size_t)source_span(a) * probs_itemsize(a.in_dtype);
  SMESH_TRY(stage.reserve(std::max<size_t>(bytes, 16)));
  SMESH_HIP(hipMemcpyAsync(stage.ptr, a.in, bytes, hipMemcpyHostToDevice, ctx->stream));
  a.in = stage.ptr;
  *staged = true;
  return SMESH_OK;
}

// Are the source's base and pixel strides aligned for loads of `bytes` (a power of two) of EB-byte elements?
bool source_aligned(const RsArgs& a, size_t EB, size_t bytes) {
  return reinterpret_cast<uintptr_t>(a.in) % bytes == 0 && ((uint64_t)a.s0 * EB) % bytes == 0 && ((uint64_t)a.s1 * EB) % bytes == 0;
}

dim3 column_grid(const RsArgs& a, uint64_t per_column) {
  return dim3((uint32_t)div_up(per_column, kRsBlock), std::min<uint32_t>(a.W, kMaxGridY));
}

// Queues k_resize_probs on the context's main stream.  Context locked, device current, `a` checked and on the device.
int launch_resize(DeviceCtx* ctx, RsArgs a) {
  const size_t ieb = probs_itemsize(a.in_dtype), oeb = probs_itemsize(a.out_dtype);
  const uint32_t VE = (uint32_t)(16 / oeb);
  const bool vec = opt_resize_vector() && a.s2 == 1 && a.C % VE == 0 && source_aligned(a, ieb, std::min<size_t>(VE * ieb, 16)) &&
                   reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && (uint64_t)a.H * (a.C / VE) < 0x80000000ull;
  const dim3 b(kRsBlock);
  if (vec) {
    a.CV = a.C / VE;
    a.col = (uint64_t)a.H * a.CV;
    const dim3 g = column_grid(a, a.col);
    if (ieb == 4 && oeb == 4) hipLaunchKernelGGL((k_resize_probs<4, 4>), g, b, 0, ctx->stream, a);
    else if (ieb == 4) hipLaunchKernelGGL((k_resize_probs<4, 2>), g, b, 0, ctx->stream, a);
    else if (oeb == 4) hipLaunchKernelGGL((k_resize_probs<2, 4>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_resize_probs<2, 2>), g, b, 0, ctx->stream, a);
  } else {
    a.col = (uint64_t)a.H * a.C;
    if (div_up(a.col, kRsBlock) > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "image too large");
    hipLaunchKernelGGL(k_resize_probs_generic, column_grid(a, a.col), b, 0, ctx->stream, a);
  }
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// Queues k_resize_probs_labels on the context's main stream: writes a.lbl and / or a.lbl32.
int launch_resize_labels(DeviceCtx* ctx, const RsArgs& a) {
  const size_t eb = probs_itemsize(a.in_dtype);
  const bool vec = opt_resize_vector() && a.s2 == 1 && a.C >= 16 / eb && source_aligned(a, eb, 16);
  const dim3 g = column_grid(a, a.H), b(kRsBlock);
  if (eb == 4) {
    if (vec) hipLaunchKernelGGL((k_resize_probs_labels<4, true>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_resize_probs_labels<4, false>), g, b, 0, ctx->stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_resize_probs_labels<2, true>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_resize_probs_labels<2, false>), g, b, 0, ctx->stream, a);
  }
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

uint64_t label_span_bytes(const RsArgs& a, uint64_t W, uint64_t H) {
  return (1 + (W - 1) * (uint64_t)a.os0 + (H - 1) * (uint64_t)a.os1) * label_itemsize(a.lbl_dtype);
}

struct ScratchGuard {     // scratch of one call
  Scratch s;
  ~ScratchGuard() { s.release(); }
};

}  // namespace

extern "C" {

int smesh_resize_probs(const void* in, int in_dtype, const int64_t in_strides[3], int in_mem, uint64_t w, uint64_t h, uint32_t C,
                       void* out, int out_dtype, uint64_t W, uint64_t H, int mode, int device) {
  if (W == 0 || H == 0) return SMESH_OK;
  RsArgs a = {};
  SMESH_TRY(check_source(a, "resize probs", in, in_dtype, in_strides, in_mem, w, h, C, W, H, mode));
  if (!out) return fail(SMESH_ERR_INVALID, "resize probs: NULL output image");
  if (bad_probs_dtype(out_dtype)) return fail(SMESH_ERR_INVALID, "resize probs: bad output dtype");
  if (reinterpret_cast<uintptr_t>(out) % probs_itemsize(out_dtype)) return fail(SMESH_ERR_INVALID, "resize probs: the output is not aligned to its element size");
  SMESH_TRY(check_no_overlap("resize probs", a, out, W * H * (uint64_t)C * probs_itemsize(out_dtype)));
  a.out = out;
  a.out_dtype = out_dtype;
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  ScratchGuard src;
  bool staged = false;
  SMESH_TRY(source_on_device(ctx, src.s, a, in_mem, &staged));
  SMESH_TRY(launch_resize(ctx, a));
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

int smesh_resize_probs_labels(const void* in, int in_dtype, const int64_t in_strides[3], int in_mem, uint64_t w, uint64_t h, uint32_t C,
                              float dont_care_threshold, void* out, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value,
                              uint64_t W, uint64_t H, int mode, int device) {
  if (W == 0 || H == 0) return SMESH_OK;
  RsArgs a = {};
  SMESH_TRY(check_source(a, "resize probs labels", in, in_dtype, in_strides, in_mem, w, h, C, W, H, mode));
  if (!out) return fail(SMESH_ERR_INVALID, "resize probs labels: NULL label image");
  a.lbl = out;
  SMESH_TRY(check_labels_out(a, "resize probs labels", out_dtype, out_strides, dont_care_value, H, C, dont_care_threshold));
  SMESH_TRY(check_no_overlap("resize probs labels", a, out, label_span_bytes(a, W, H)));
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  ScratchGuard src;
  bool staged = false;
  SMESH_TRY(source_on_device(ctx, src.s, a, in_mem, &staged));
  SMESH_TRY(launch_resize_labels(ctx, a));
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

int smesh_confusion_add_probs_resized(smesh_confusion_t* cm, const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_mem,
                                      uint64_t w, uint64_t h, const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_mem,
                                      uint64_t W, uint64_t H, float dont_care_threshold, int mode, void* labels_out, int out_dtype,
                                      const int64_t out_strides[2], int64_t dont_care_value) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  if (W == 0 || H == 0) return SMESH_OK;
  RsArgs a = {};
  SMESH_TRY(check_source(a, "confusion add probs resized", probs, probs_dtype, probs_strides, probs_mem, w, h, cm->C, W, H, mode));
  SMESH_TRY(check_gt(gt, gt_dtype, gt_strides, gt_mem));
  a.lbl = labels_out;
  SMESH_TRY(check_labels_out(a, "confusion add probs resized", out_dtype, out_strides, dont_care_value, H, cm->C, dont_care_threshold));
  if (labels_out) SMESH_TRY(check_no_overlap("confusion add probs resized", a, labels_out, label_span_bytes(a, W, H)));
  std::lock_guard<std::mutex> g(cm->mu);
  DeviceCtx* ctx = cm->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  bool staged = false;
  SMESH_TRY(source_on_device(ctx, cm->stage_src, a, probs_mem, &staged));
  const void* d_gt = nullptr;
  SMESH_TRY(image_on_device(ctx, cm->stage_gt, gt, label_itemsize(gt_dtype), gt_strides, gt_mem, W, H, &d_gt, &staged));
  // int32 labels into scratch, then k_confusion in its labels mode: the two-launch form of smesh_confusion_add_probs
  SMESH_TRY(cm->stage_lbl.reserve((size_t)(W * H) * 4));
  a.lbl32 = static_cast<int32_t*>(cm->stage_lbl.ptr);
  SMESH_TRY(launch_resize_labels(ctx, a));
  SMESH_TRY(smesh_confusion_count_label_image(cm, a.lbl32, d_gt, gt_dtype, gt_strides, W, H));
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

}  // extern "C"
