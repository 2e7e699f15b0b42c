// lens.hip -- images from cameras with lens distortion, undistorted on the device (include/smesh_lens.h): the dense (W,H,C)
// class-vector image of the pinhole view with its validity weights plane, and the nearest-sampled (W,H[,channels]) image of masks,
// colour masks and sensor depth.
//
// Reference: eval-scannet/run_colmap_on_scannet.py:108 (`colmap image_undistorter` before anything is segmented or fused) -- the
// reference itself has no counterpart.
//
// The rule is evaluated in ONE place, lens_tap() / lens_axis() / lens_nearest() of lens_rule.hpp, and the blend is
// blend() of resize_rule.hpp: coordinates in double, the three lerps in float32, every operation rounded separately (the library
// is built with -ffp-contract=off).  No result depends on the path, the dtype pair's load width or the launch shape.
#include "half_scratch.hpp"
#include "lens_rule.hpp"

#include <atomic>
#include <cmath>
#include <cstring>

#include "../../include/smesh_lens.h"

#pragma clang fp contract(off)

using namespace smesh;

namespace {

constexpr int kLnBlock = 256;
constexpr uint32_t kXcds = 8;       // accelerator dies of the MI355X: consecutive workgroups of a launch go to them in turn
constexpr int kCounts = 2;          // pixels, outside

std::atomic<uint64_t> g_launches{0};
thread_local int g_last_path = 0;   // the calling thread's last launch: 0 none, 1 vector, 2 generic, 3 pixels ("last_lens_path")

size_t probs_itemsize(int dt) { return dt == SMESH_PROBS_F32 ? 4 : 2; }
bool bad_probs_dtype(int dt) { return dt != SMESH_PROBS_F32 && dt != SMESH_PROBS_F16 && dt != SMESH_PROBS_BF16; }

typedef uint32_t ln_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ln_u32x2 __attribute__((ext_vector_type(2)));

struct LnArgs {
  LensMap m;
  const void* in;
  int64_t s0, s1, s2;           // element strides of x, y and the class / channel of `in`
  uint32_t W, H, C;
  int in_dtype;
  void* out;                    // dense (W,H,C) of out_dtype, or dense (W,H[,ch])
  int out_dtype;
  uint32_t CV;                  // vector path: 16-byte pieces of a pixel's row
  uint64_t col;                 // work items of one output column: H CV pieces, or H C elements
  uint32_t bpc;                 // workgroups per output column
  uint64_t chunks;              // workgroups with work: W bpc, or ceil(W H / 256) of the pixel kernel
  const float* w_in;            // dense (W,H), or null: 1.0f
  float* w_out;                 // dense (W,H), or null
  unsigned long long* counts;   // [kCounts], or null
  uint32_t ch;                  // smesh_undistort_pixels: channels, and the fill pixel's elements (low bytes)
  uint64_t fill[4];
};

// Workgroups go to the eight XCDs in turn (gridDim.x is a multiple of eight): XCD j takes the j-th run of consecutive chunks, so the
// source lines that neighbouring output columns share are fetched into one L2 and not into all eight (the mapping k_depth_weights
// measured and kept).
__device__ __forceinline__ uint64_t chunk_of() {
  const uint32_t per_xcd = gridDim.x / kXcds;
  return (uint64_t)(blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds;
}

// One atomic per wave and counter.  Every lane of the wave calls this with the wave's own totals.
__device__ __forceinline__ void add_counts(unsigned long long* counts, uint32_t pixels, uint32_t outside) {
  if (counts && (threadIdx.x & 63u) == 0u) {
    if (pixels) atomicAdd(&counts[0], (unsigned long long)pixels);
    if (outside) atomicAdd(&counts[1], (unsigned long long)outside);
  }
}

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
      const ln_u32x4 q = *reinterpret_cast<const ln_u32x4*>(p + k * 4);
      v[k] = __uint_as_float(q.x); v[k + 1] = __uint_as_float(q.y); v[k + 2] = __uint_as_float(q.z); v[k + 3] = __uint_as_float(q.w);
    }
  } else if constexpr (VE == 8) {
    const ln_u32x4 q = *reinterpret_cast<const ln_u32x4*>(p);
    unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]); unpack2(q.z, bf, v[4], v[5]); unpack2(q.w, bf, v[6], v[7]);
  } else {
    const ln_u32x2 q = *reinterpret_cast<const ln_u32x2*>(p);
    unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]);
  }
}

// The weight of pixel (X, Y), written by the one lane that owns the pixel.
__device__ __forceinline__ void store_weight(const LnArgs& a, uint32_t X, uint32_t Y, bool inside) {
  if (!a.w_out) return;
  const uint64_t i = (uint64_t)X * a.H + Y;
  a.w_out[i] = inside ? (a.w_in ? a.w_in[i] : 1.0f) : 0.0f;
}

// VECTOR path: k_resize_probs' shape -- a lane owns 16 bytes of the dense output, VE = 16 / OEB classes of one pixel, and lanes run
// along the output's memory order inside a column (y, then the class), so a wave's stores are 1 KiB contiguous.  The C OEB / 16 lanes
// that share a pixel share its map, which is about thirty double operations and a division: the workgroup first computes the map of
// its run of pixels -- at most 256, when a pixel is one piece --, one lane per pixel, into LDS; after one barrier the lanes blend.
// LDS: five arrays of 256 dwords, indexed by the pixel of the run; consecutive lanes read the same or the next dword of an array
// (broadcast, or consecutive banks): no conflicts, 5 KiB a workgroup.  A pixel whose pieces straddle two workgroups is mapped by
// both and OWNED (its weight, its counts) by the one that holds its first piece.
template <int IEB, int OEB>
__global__ __launch_bounds__(kLnBlock) void k_undistort_probs(LnArgs a) {
  constexpr int VE = 16 / OEB;
  __shared__ uint32_t s_x[kLnBlock], s_y[kLnBlock], s_inside[kLnBlock];
  __shared__ float s_fx[kLnBlock], s_fy[kLnBlock];
  const uint64_t chunk = chunk_of();
  if (chunk >= a.chunks) return;                                    // (uniform over the workgroup)
  const uint32_t X = (uint32_t)(chunk / a.bpc), b = (uint32_t)(chunk - (uint64_t)X * a.bpc);
  const uint32_t first = b * kLnBlock;                              // (a.col < 2^31)
  const uint32_t last = min(first + (uint32_t)kLnBlock - 1u, (uint32_t)a.col - 1u);
  const uint32_t Ylo = first / a.CV, Yhi = last / a.CV;             // Yhi - Ylo < 256
  {
    const uint32_t Y = Ylo + threadIdx.x;
    const bool have = Y <= Yhi;
    const bool own = have && Y * a.CV >= first;
    bool inside = false;
    if (have) {
      const LensTap t = lens_tap(a.m, X, Y);
      inside = t.inside;
      Axis ax = {0u, 0u, 0.0f}, ay = {0u, 0u, 0.0f};
      if (inside) { ax = lens_axis(t.tx, a.m.w); ay = lens_axis(t.ty, a.m.h); }
      s_x[threadIdx.x] = ax.i0 | (ax.i1 << 16);                     // (indices <= 65535)
      s_y[threadIdx.x] = ay.i0 | (ay.i1 << 16);
      s_fx[threadIdx.x] = ax.f;
      s_fy[threadIdx.x] = ay.f;
      s_inside[threadIdx.x] = inside ? 1u : 0u;
      if (own) store_weight(a, X, Y, inside);
    }
    if (a.counts)                                                   // (uniform: every lane of a wave reaches the ballots)
      add_counts(a.counts, (uint32_t)__popcll(__ballot(own)), (uint32_t)__popcll(__ballot(own && !inside)));
  }
  __syncthreads();
  const uint32_t v = first + threadIdx.x;
  if (v > last) return;
  const uint32_t Y = v / a.CV, c = (v - Y * a.CV) * VE, e = Y - Ylo;
  const uint32_t px = s_x[e], py = s_y[e];
  const float fx = s_fx[e], fy = s_fy[e];
  const bool inside = s_inside[e] != 0u;
  const bool ibf = a.in_dtype == SMESH_PROBS_BF16, obf = a.out_dtype == SMESH_PROBS_BF16;
  ln_u32x4 q = {0u, 0u, 0u, 0u};                                    // an outside row: all +0.0f, in every dtype
  if (inside) {
    const char* in = static_cast<const char*>(a.in);
    const uint64_t c0 = (uint64_t)(px & 0xFFFFu) * (uint64_t)a.s0, c1 = (uint64_t)(px >> 16) * (uint64_t)a.s0;
    const uint64_t r0 = (uint64_t)(py & 0xFFFFu) * (uint64_t)a.s1 + c, r1 = (uint64_t)(py >> 16) * (uint64_t)a.s1 + c;
    float a00[VE], a10[VE], a01[VE], a11[VE];
    load_row<IEB, VE>(in + (c0 + r0) * IEB, ibf, a00);
    load_row<IEB, VE>(in + (c1 + r0) * IEB, ibf, a10);
    load_row<IEB, VE>(in + (c0 + r1) * IEB, ibf, a01);
    load_row<IEB, VE>(in + (c1 + r1) * IEB, ibf, a11);
    float r[VE];
#pragma unroll
    for (int k = 0; k < VE; k++) r[k] = blend(a00[k], a10[k], a01[k], a11[k], fx, fy);
    if constexpr (OEB == 4) {
      q.x = __float_as_uint(r[0]); q.y = __float_as_uint(r[1]); q.z = __float_as_uint(r[2]); q.w = __float_as_uint(r[3]);
    } else {
      q.x = narrow1(r[0], obf) | (narrow1(r[1], obf) << 16); q.y = narrow1(r[2], obf) | (narrow1(r[3], obf) << 16);
      q.z = narrow1(r[4], obf) | (narrow1(r[5], obf) << 16); q.w = narrow1(r[6], obf) | (narrow1(r[7], obf) << 16);
    }
  }
  const uint64_t o = ((uint64_t)X * a.H + Y) * a.C + c;
  *reinterpret_cast<ln_u32x4*>(static_cast<char*>(a.out) + o * OEB) = q;
}

// GENERIC path: any strides, class count and alignment.  One lane per output element, which maps its own pixel; the lane of class 0
// owns the pixel.  Correct, not fast.
__global__ __launch_bounds__(kLnBlock) void k_undistort_probs_generic(LnArgs a) {
  const uint64_t chunk = chunk_of();
  if (chunk >= a.chunks) return;                                    // (uniform over the workgroup)
  const uint32_t X = (uint32_t)(chunk / a.bpc), b = (uint32_t)(chunk - (uint64_t)X * a.bpc);
  const uint64_t e = (uint64_t)b * kLnBlock + threadIdx.x;
  const bool have = e < a.col;
  uint32_t Y = 0u, c = 0u;
  bool inside = false;
  if (have) {
    Y = (uint32_t)(e / a.C);
    c = (uint32_t)(e - (uint64_t)Y * a.C);
    const LensTap t = lens_tap(a.m, X, Y);
    inside = t.inside;
    float r = 0.0f;
    if (inside) {
      const Axis ax = lens_axis(t.tx, a.m.w), ay = lens_axis(t.ty, a.m.h);
      const uint64_t c0 = (uint64_t)ax.i0 * (uint64_t)a.s0, c1 = (uint64_t)ax.i1 * (uint64_t)a.s0;
      const uint64_t r0 = (uint64_t)ay.i0 * (uint64_t)a.s1 + (uint64_t)c * (uint64_t)a.s2;
      const uint64_t r1 = (uint64_t)ay.i1 * (uint64_t)a.s1 + (uint64_t)c * (uint64_t)a.s2;
      r = blend(load_elem(a.in, a.in_dtype, c0 + r0), load_elem(a.in, a.in_dtype, c1 + r0),
                load_elem(a.in, a.in_dtype, c0 + r1), load_elem(a.in, a.in_dtype, c1 + r1), ax.f, ay.f);
    }
    const uint64_t o = (uint64_t)X * a.col + e;
    if (a.out_dtype == SMESH_PROBS_F32) static_cast<float*>(a.out)[o] = r;
    else static_cast<uint16_t*>(a.out)[o] = (uint16_t)narrow1(r, a.out_dtype == SMESH_PROBS_BF16);
    if (c == 0u) store_weight(a, X, Y, inside);
  }
  if (a.counts) {
    const bool own = have && c == 0u;
    add_counts(a.counts, (uint32_t)__popcll(__ballot(own)), (uint32_t)__popcll(__ballot(own && !inside)));
  }
}

// NEAREST: one lane per output pixel, lanes along the output's memory order (y, then x), a workgroup takes 256 consecutive pixels.
// T: an unsigned integer of the element's size -- the pixel is moved, not interpreted.
template <typename T>
__global__ __launch_bounds__(kLnBlock) void k_undistort_pixels(LnArgs a) {
  const uint64_t chunk = chunk_of();
  if (chunk >= a.chunks) return;                                    // (uniform over the workgroup)
  const uint32_t N = a.W * a.H;                                     // (< 2^29)
  const uint32_t i = (uint32_t)chunk * kLnBlock + threadIdx.x;
  const bool have = i < N;
  bool inside = false;
  if (have) {
    const uint32_t X = i / a.H, Y = i - X * a.H;
    const LensTap t = lens_tap(a.m, X, Y);
    inside = t.inside;
    T* out = static_cast<T*>(a.out) + (uint64_t)i * a.ch;
    if (inside) {
      const T* in = static_cast<const T*>(a.in) + (uint64_t)lens_nearest(t.tx, a.m.w) * (uint64_t)a.s0 + (uint64_t)lens_nearest(t.ty, a.m.h) * (uint64_t)a.s1;
      T px[4] = {0, 0, 0, 0};                                        // the loads ahead of the stores, all in registers
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (k < a.ch) px[k] = in[(uint64_t)k * (uint64_t)a.s2];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (k < a.ch) out[k] = px[k];
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (k < a.ch) out[k] = (T)a.fill[k];
    }
  }
  if (a.counts) add_counts(a.counts, (uint32_t)__popcll(__ballot(have)), (uint32_t)__popcll(__ballot(have && !inside)));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// The checks both entry points share about the lens, the view and the sizes; fills a.m, a.W and a.H.
int check_geometry(LnArgs& a, const char* who, const smesh_lens_t* lens, const smesh_camera_t* view, uint64_t w, uint64_t h) {
  const std::string p = std::string(who) + ": ";
  if (!lens || !view) return fail(SMESH_ERR_INVALID, p + "NULL lens or view camera");
  if (!finite_all(lens->focal, 2) || !finite_all(lens->principal, 2) || !finite_all(lens->k, 6) || !finite_all(lens->p, 2))
    return fail(SMESH_ERR_INVALID, p + "a lens parameter is not finite");
  if (!finite_all(view->focal, 2) || !finite_all(view->principal, 2)) return fail(SMESH_ERR_INVALID, p + "a view camera parameter is not finite");
  if (!(lens->focal[0] > 0.0) || !(lens->focal[1] > 0.0) || !(view->focal[0] > 0.0) || !(view->focal[1] > 0.0))
    return fail(SMESH_ERR_INVALID, p + "focal lengths must be > 0");
  if (lens->width == 0 || lens->height == 0) return fail(SMESH_ERR_INVALID, p + "the lens has an empty calibration size");
  if (w == 0 || h == 0) return fail(SMESH_ERR_INVALID, p + "an empty source image cannot fill a non-empty target");
  if (w > 65536 || h > 65536 || lens->width > 65536 || lens->height > 65536) return fail(SMESH_ERR_INVALID, "image too large");
  if (view->width > 65536 || view->height > 65536 || view->width * view->height >= (1ull << 29)) return fail(SMESH_ERR_INVALID, "image too large");
  LensMap& m = a.m;
  m.Fx = view->focal[0]; m.Fy = view->focal[1]; m.Px = view->principal[0]; m.Py = view->principal[1];
  m.fx = lens->focal[0]; m.fy = lens->focal[1]; m.cx = lens->principal[0]; m.cy = lens->principal[1];
  m.k1 = lens->k[0]; m.k2 = lens->k[1]; m.k3 = lens->k[2]; m.k4 = lens->k[3]; m.k5 = lens->k[4]; m.k6 = lens->k[5];
  m.p1 = lens->p[0]; m.p2 = lens->p[1];
  m.p1x2 = 2.0 * lens->p[0]; m.p2x2 = 2.0 * lens->p[1];
  m.rx = (double)w / (double)lens->width;
  m.ry = (double)h / (double)lens->height;
  m.xmax = (double)w - 0.5;
  m.ymax = (double)h - 0.5;
  m.w = (uint32_t)w; m.h = (uint32_t)h;
  m.rational = (m.k4 != 0.0 || m.k5 != 0.0 || m.k6 != 0.0) ? 1u : 0u;
  a.W = (uint32_t)view->width;
  a.H = (uint32_t)view->height;
  return SMESH_OK;
}

// Elements that the strides of the source cover (C: classes or channels).
uint64_t source_span(const LnArgs& a, uint32_t C) {
  return 1 + (uint64_t)(a.m.w - 1) * (uint64_t)a.s0 + (uint64_t)(a.m.h - 1) * (uint64_t)a.s1 + (uint64_t)(C - 1) * (uint64_t)a.s2;
}

bool overlaps(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// A HOST source staged at its own size and width: the span its strides cover.
int source_on_device(DeviceCtx* ctx, Scratch& stage, LnArgs& a, size_t bytes, int mem, bool* staged) {
  if (mem == SMESH_MEM_DEVICE) return SMESH_OK;
  SMESH_TRY(stage.reserve(std::max<size_t>(bytes, 16)));
  SMESH_HIP(hipMemcpyAsync(stage.ptr, a.in, bytes, hipMemcpyHostToDevice, ctx->stream));
  a.in = stage.ptr;
  *staged = true;
  return SMESH_OK;
}

bool source_aligned(const LnArgs& a, size_t EB, size_t bytes) {
  return reinterpret_cast<uintptr_t>(a.in) % bytes == 0 && ((uint64_t)a.s0 * EB) % bytes == 0 && ((uint64_t)a.s1 * EB) % bytes == 0;
}

// The grid of a.chunks workgroups, rounded up to the XCDs; refuses what a launch cannot hold.
int xcd_grid(const LnArgs& a, dim3* g) {
  const uint64_t n = kXcds * div_up(a.chunks, kXcds);
  if (n > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "image too large");
  *g = dim3((uint32_t)n);
  return SMESH_OK;
}

// Queues k_undistort_probs on the context's main stream.  Context locked, device current, `a` checked and on the device.
int launch_probs(DeviceCtx* ctx, LnArgs a) {
  const size_t ieb = probs_itemsize(a.in_dtype), oeb = probs_itemsize(a.out_dtype);
  const uint32_t VE = (uint32_t)(16 / oeb);
  // (the conditions of launch_resize, resize.hip)
  const bool vec = opt_lens_vector() && a.s2 == 1 && a.C % VE == 0 && source_aligned(a, ieb, std::min<size_t>(VE * ieb, 16)) &&
                   reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && (uint64_t)a.H * (a.C / VE) < 0x80000000ull;
  const dim3 b(kLnBlock);
  dim3 g;
  if (vec) {
    a.CV = a.C / VE;
    a.col = (uint64_t)a.H * a.CV;
  } else {
    a.col = (uint64_t)a.H * a.C;
    if (div_up(a.col, kLnBlock) > 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "image too large");
  }
  a.bpc = (uint32_t)div_up(a.col, kLnBlock);
  a.chunks = (uint64_t)a.W * a.bpc;
  SMESH_TRY(xcd_grid(a, &g));
  if (!vec) hipLaunchKernelGGL(k_undistort_probs_generic, g, b, 0, ctx->stream, a);
  else if (ieb == 4 && oeb == 4) hipLaunchKernelGGL((k_undistort_probs<4, 4>), g, b, 0, ctx->stream, a);
  else if (ieb == 4) hipLaunchKernelGGL((k_undistort_probs<4, 2>), g, b, 0, ctx->stream, a);
  else if (oeb == 4) hipLaunchKernelGGL((k_undistort_probs<2, 4>), g, b, 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_undistort_probs<2, 2>), g, b, 0, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  g_last_path = vec ? 1 : 2;
  return SMESH_OK;
}

int launch_pixels(DeviceCtx* ctx, LnArgs a, int eb) {
  a.chunks = div_up((uint64_t)a.W * a.H, kLnBlock);
  dim3 g;
  SMESH_TRY(xcd_grid(a, &g));
  const dim3 b(kLnBlock);
  if (eb == 1) hipLaunchKernelGGL(k_undistort_pixels<uint8_t>, g, b, 0, ctx->stream, a);
  else if (eb == 2) hipLaunchKernelGGL(k_undistort_pixels<uint16_t>, g, b, 0, ctx->stream, a);
  else if (eb == 4) hipLaunchKernelGGL(k_undistort_pixels<uint32_t>, g, b, 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_undistort_pixels<uint64_t>, g, b, 0, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  g_last_path = 3;
  return SMESH_OK;
}

struct ScratchGuard {     // scratch of one call
  Scratch s;
  ~ScratchGuard() { s.release(); }
};

// Zeroed device counters ahead of a launch, when the caller asked for counts.
int counts_begin(DeviceCtx* ctx, Scratch& s, LnArgs& a, uint64_t* counts) {
  if (!counts) return SMESH_OK;
  SMESH_TRY(s.reserve(16));
  SMESH_HIP(hipMemsetAsync(s.ptr, 0, sizeof(unsigned long long) * kCounts, ctx->stream));
  a.counts = static_cast<unsigned long long*>(s.ptr);
  return SMESH_OK;
}

// Waits where the call must: for the counts, and for a staged host source (host arrays are consumed before the call returns).
int finish(DeviceCtx* ctx, const LnArgs& a, uint64_t* counts, bool staged) {
  if (counts) SMESH_HIP(hipMemcpyAsync(counts, a.counts, sizeof(unsigned long long) * kCounts, hipMemcpyDeviceToHost, ctx->stream));
  if (counts || staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));
  return SMESH_OK;
}

}  // namespace

// (context.cpp: the read-only option "lens_launches")
namespace smesh {
uint64_t smesh_lens_launches() { return g_launches.load(); }
int smesh_last_lens_path() { return g_last_path; }
}  // namespace smesh

extern "C" {

int smesh_undistort_probs(const void* in, int in_dtype, const int64_t in_strides[3], int in_mem, uint64_t w, uint64_t h, uint32_t C,
                          const smesh_lens_t* lens, const smesh_camera_t* view, void* out, int out_dtype, const float* weights_in,
                          float* weights_out, uint64_t* counts, int device) {
  const char* who = "undistort probs";
  const std::string p = std::string(who) + ": ";
  LnArgs a = {};
  if (!in) return fail(SMESH_ERR_INVALID, p + "NULL class-vector image");
  if (bad_probs_dtype(in_dtype)) return fail(SMESH_ERR_INVALID, p + "bad class-vector dtype");
  if (bad_probs_dtype(out_dtype)) return fail(SMESH_ERR_INVALID, p + "bad output dtype");
  if (in_strides && (in_strides[0] < 0 || in_strides[1] < 0 || in_strides[2] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (in_mem != SMESH_MEM_HOST && in_mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (reinterpret_cast<uintptr_t>(in) % probs_itemsize(in_dtype)) return fail(SMESH_ERR_INVALID, p + "the image is not aligned to its element size");
  if (C == 0) return fail(SMESH_ERR_INVALID, p + "the class count must be positive");
  SMESH_TRY(check_geometry(a, who, lens, view, w, h));
  if (a.W == 0 || a.H == 0) {
    if (counts) counts[0] = counts[1] = 0;
    return SMESH_OK;
  }
  if (!out) return fail(SMESH_ERR_INVALID, p + "NULL output image");
  if (reinterpret_cast<uintptr_t>(out) % probs_itemsize(out_dtype)) return fail(SMESH_ERR_INVALID, p + "the output is not aligned to its element size");
  if (weights_in && !weights_out) return fail(SMESH_ERR_INVALID, p + "a weights image to multiply needs a weights plane to write");
  if ((reinterpret_cast<uintptr_t>(weights_in) | reinterpret_cast<uintptr_t>(weights_out)) % 4) return fail(SMESH_ERR_INVALID, p + "a weights plane is not aligned to its element size");
  a.in = in;
  a.in_dtype = in_dtype;
  a.s0 = in_strides ? in_strides[0] : (int64_t)(h * C);
  a.s1 = in_strides ? in_strides[1] : (int64_t)C;
  a.s2 = in_strides ? in_strides[2] : 1;
  a.C = C;
  const uint64_t in_bytes = source_span(a, C) * probs_itemsize(in_dtype), pixels = (uint64_t)a.W * a.H;
  const uint64_t out_bytes = pixels * C * probs_itemsize(out_dtype);
  if (in_mem == SMESH_MEM_DEVICE && (overlaps(in, in_bytes, out, out_bytes) || overlaps(in, in_bytes, weights_out, pixels * 4)))
    return fail(SMESH_ERR_INVALID, p + "an output overlaps the input");
  if (overlaps(out, out_bytes, weights_out, pixels * 4) || overlaps(out, out_bytes, weights_in, pixels * 4))
    return fail(SMESH_ERR_INVALID, p + "the output image overlaps a weights plane");
  if (counts) counts[0] = counts[1] = 0;      // (behind the last refusal: a refused call leaves nothing changed)
  a.out = out;
  a.out_dtype = out_dtype;
  a.w_in = weights_in;
  a.w_out = weights_out;
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  ScratchGuard src, cnt;
  bool staged = false;
  SMESH_TRY(source_on_device(ctx, src.s, a, (size_t)in_bytes, in_mem, &staged));
  SMESH_TRY(counts_begin(ctx, cnt.s, a, counts));
  SMESH_TRY(launch_probs(ctx, a));
  return finish(ctx, a, counts, staged);
}

int smesh_undistort_pixels(const void* in, int elem_bytes, int channels, const int64_t in_strides[3], int in_mem, uint64_t w, uint64_t h,
                           const smesh_lens_t* lens, const smesh_camera_t* view, const void* fill, void* out, uint64_t* counts, int device) {
  const char* who = "undistort pixels";
  const std::string p = std::string(who) + ": ";
  LnArgs a = {};
  if (!in || !fill) return fail(SMESH_ERR_INVALID, p + "NULL image or fill pixel");
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return fail(SMESH_ERR_INVALID, p + "elements must be of 1, 2, 4 or 8 bytes");
  if (channels < 1 || channels > 4) return fail(SMESH_ERR_INVALID, p + "pixels must have 1 to 4 channels");
  if (in_strides && (in_strides[0] < 0 || in_strides[1] < 0 || (channels > 1 && in_strides[2] < 0)))
    return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (in_mem != SMESH_MEM_HOST && in_mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (reinterpret_cast<uintptr_t>(in) % (size_t)elem_bytes) return fail(SMESH_ERR_INVALID, p + "the image is not aligned to its element size");
  SMESH_TRY(check_geometry(a, who, lens, view, w, h));
  if (a.W == 0 || a.H == 0) {
    if (counts) counts[0] = counts[1] = 0;
    return SMESH_OK;
  }
  if (!out) return fail(SMESH_ERR_INVALID, p + "NULL output image");
  if (reinterpret_cast<uintptr_t>(out) % (size_t)elem_bytes) return fail(SMESH_ERR_INVALID, p + "the output is not aligned to its element size");
  a.in = in;
  a.s0 = in_strides ? in_strides[0] : (int64_t)(h * (uint64_t)channels);
  a.s1 = in_strides ? in_strides[1] : (int64_t)channels;
  a.s2 = channels > 1 ? (in_strides ? in_strides[2] : 1) : 0;
  a.ch = (uint32_t)channels;
  for (int k = 0; k < channels; k++) memcpy(&a.fill[k], static_cast<const char*>(fill) + (size_t)k * (size_t)elem_bytes, (size_t)elem_bytes);
  const uint64_t in_bytes = source_span(a, (uint32_t)channels) * (uint64_t)elem_bytes;
  const uint64_t out_bytes = (uint64_t)a.W * a.H * (uint64_t)channels * (uint64_t)elem_bytes;
  if (in_mem == SMESH_MEM_DEVICE && overlaps(in, in_bytes, out, out_bytes)) return fail(SMESH_ERR_INVALID, p + "the output overlaps the input");
  if (counts) counts[0] = counts[1] = 0;      // (behind the last refusal: a refused call leaves nothing changed)
  a.out = out;
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  ScratchGuard src, cnt;
  bool staged = false;
  SMESH_TRY(source_on_device(ctx, src.s, a, (size_t)in_bytes, in_mem, &staged));
  SMESH_TRY(counts_begin(ctx, cnt.s, a, counts));
  SMESH_TRY(launch_pixels(ctx, a, elem_bytes));
  return finish(ctx, a, counts, staged);
}

}  // extern "C"
