// label_prep.hip -- a label image at its own resolution and in the dataset's ids -> the dense (W,H) plane the label fusion and the
// confusion matrices read: k_labels_prepare, its launcher and smesh_labels_prepare (include/smesh_label_prep.h, where the rule is
// stated to the bit).  The prepared fusion entry points of that header live beside their counterparts in fusion_labels.hip and call
// smesh_label_prep_launch from narrow_plane().
//
// Per output pixel (X, Y):  sx = ((2X + 1) w) div (2W),  sy = ((2Y + 1) h) div (2H)   (integers; no floating point anywhere)
//                           v  = in[sx * s0 + sy * s1]
//                           v  = map[v] if a map is given (v outside [0, M): don't care)
//                           out[X * H + Y] = v in [0, C) ? v : all ones
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "labels_scratch.hpp"
#include "nearest_rule.hpp"
#include "../../include/smesh_label_prep.h"

#include <atomic>
#include <mutex>
#include <type_traits>

using namespace smesh;

namespace {

constexpr uint32_t kMapLdsMax = SMESH_LABEL_PREP_MAP_LDS_MAX;   // entries of a map kept in LDS
constexpr uint32_t kChunk = 4096;                               // output pixels per workgroup (one LDS map copy serves them)

std::atomic<uint64_t> g_launches{0};

struct PrepArgs {
  const void* in;
  int64_t s0, s1;             // element strides of the source
  uint32_t w, h, W, H;
  uint32_t C, M;              // M: entries of the map (0 without one)
  const int32_t* map;         // device memory, or null
  void* out;
  uint32_t map_lds;           // the map is copied into LDS as narrowed codes
};

// (the rule, per axis: src_index, nearest_rule.hpp)

template <typename T>
__device__ __forceinline__ bool in_range(T v, uint32_t limit) {
  bool ok = (uint64_t)v < (uint64_t)limit;
  if (std::is_signed<T>::value) ok = ok && !(v < (T)0);
  return ok;
}

// The map as narrowed codes (65535: don't care; as uint8, 255), once per workgroup.  The caller synchronises.
__device__ __forceinline__ void fill_map(const PrepArgs& a, uint16_t* __restrict__ lmap) {
  if (!a.map_lds) return;
  for (uint32_t i = threadIdx.x; i < a.M; i += blockDim.x) {
    const int32_t m = a.map[i];
    lmap[i] = (m >= 0 && (uint32_t)m < a.C) ? (uint16_t)m : (uint16_t)0xFFFFu;
  }
}

// map, then narrow
template <typename T, typename OUT>
__device__ __forceinline__ OUT code_of(T v, const PrepArgs& a, const uint16_t* __restrict__ lmap) {
  constexpr OUT kDontCare = (OUT)~(OUT)0;
  if (a.map) {
    if (!in_range(v, a.M)) return kDontCare;
    if (a.map_lds) return (OUT)lmap[(uint32_t)v];   // (a uint8 plane has C <= 255: every class code fits, 65535 becomes 255)
    const int32_t m = a.map[(uint32_t)v];
    return (m >= 0 && (uint32_t)m < a.C) ? (OUT)m : kDontCare;
  }
  return in_range(v, a.C) ? (OUT)v : kDontCare;
}

// One lane per output pixel, lanes along the output's y (k_labels_narrow's structure); a workgroup takes kChunk consecutive pixels.
// Serves every layout and every ratio.  (A second form that staged the source rectangle of a 64 x 64 output tile in LDS, for sources
// whose fastest axis is x, was measured against this one and removed: DESIGN.md 3.10.)
template <typename T, typename OUT>
__global__ __launch_bounds__(256) void k_labels_prepare(PrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* lmap = reinterpret_cast<uint16_t*>(smem);
  fill_map(a, lmap);
  if (a.map_lds) __syncthreads();
  const T* __restrict__ in = static_cast<const T*>(a.in);
  OUT* __restrict__ out = static_cast<OUT*>(a.out);
  const uint32_t N = a.W * a.H;   // (< 2^29)
  const uint32_t base = blockIdx.x * kChunk;
  for (uint32_t k = threadIdx.x; k < kChunk; k += 256u) {
    const uint32_t i = base + k;
    if (i >= N) break;
    const uint32_t X = i / a.H, Y = i - X * a.H;
    const uint64_t sx = src_index(X, a.w, a.W), sy = src_index(Y, a.h, a.H);
    out[i] = code_of<T, OUT>(in[sx * (uint64_t)a.s0 + sy * (uint64_t)a.s1], a, lmap);
  }
}

template <typename T, typename OUT>
void launch_form(const PrepArgs& a, hipStream_t st) {
  const dim3 g((uint32_t)div_up((uint64_t)a.W * a.H, kChunk)), b(256);
  hipLaunchKernelGGL((k_labels_prepare<T, OUT>), g, b, a.map_lds ? (size_t)a.M * 2 : 0, st, a);
}

template <typename OUT>
void launch_dtype(int dt, const PrepArgs& a, hipStream_t st) {
  switch (dt) {
    case SMESH_LBL_U8:  launch_form<uint8_t, OUT>(a, st); break;
    case SMESH_LBL_I8:  launch_form<int8_t, OUT>(a, st); break;
    case SMESH_LBL_U16: launch_form<uint16_t, OUT>(a, st); break;
    case SMESH_LBL_I16: launch_form<int16_t, OUT>(a, st); break;
    case SMESH_LBL_U32: launch_form<uint32_t, OUT>(a, st); break;
    case SMESH_LBL_I32: launch_form<int32_t, OUT>(a, st); break;
    case SMESH_LBL_U64: launch_form<uint64_t, OUT>(a, st); break;
    default:            launch_form<int64_t, OUT>(a, st); break;
  }
}

}  // namespace

// (context.cpp: the read-only option "labels_prepare_launches")
namespace smesh {
uint64_t smesh_label_prep_launches() { return g_launches.load(); }
}  // namespace smesh

int smesh_label_prep_check(int dt, const int64_t* strides, int mem, const LabelPrep& p, uint64_t W, uint64_t H, uint32_t C) {
  if (dt < 0 || dt > SMESH_LBL_I64) return fail(SMESH_ERR_INVALID, "bad label dtype");
  if (strides && (strides[0] < 0 || strides[1] < 0)) return fail(SMESH_ERR_INVALID, "labels: negative strides are not supported");
  if (mem != SMESH_MEM_HOST && mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (C > 65535u) return fail(SMESH_ERR_INVALID, "label images need an aggregator of at most 65535 classes");
  if (p.w > 65536 || p.h > 65536 || W > 65536 || H > 65536 || W * H >= (1ull << 29))
    return fail(SMESH_ERR_INVALID, "label image too large: at most 65536 pixels a side and fewer than 2^29 target pixels");
  if ((p.w == 0 || p.h == 0) && W != 0 && H != 0) return fail(SMESH_ERR_INVALID, "an empty label image cannot be resampled");
  if (p.map) {
    if (p.map_len == 0) return fail(SMESH_ERR_INVALID, "label map is empty");
    if (p.map_len > (1ull << 24)) return fail(SMESH_ERR_INVALID, "label map has more than 2^24 entries");
    if (p.map_mem != SMESH_MEM_HOST && p.map_mem != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind of the label map");
  } else if (p.map_len != 0) {
    return fail(SMESH_ERR_INVALID, "label map is NULL but its length is not 0");
  }
  return SMESH_OK;
}

int smesh_label_prep_launch(DeviceCtx* ctx, const void* src, int dt, const int64_t* strides, uint64_t w, uint64_t h, const int32_t* map_dev,
                            uint64_t map_len, uint32_t C, void* out, int out_bytes, uint64_t W, uint64_t H) {
  if (W == 0 || H == 0) return SMESH_OK;
  const int64_t dense[2] = {(int64_t)h, 1};
  const int64_t* s = strides ? strides : dense;
  PrepArgs a;
  a.in = src;
  a.s0 = s[0];
  a.s1 = s[1];
  a.w = (uint32_t)w; a.h = (uint32_t)h; a.W = (uint32_t)W; a.H = (uint32_t)H;
  a.C = C;
  a.M = map_dev ? (uint32_t)map_len : 0u;
  a.map = map_dev;
  a.out = out;
  a.map_lds = (map_dev && map_len <= kMapLdsMax) ? 1u : 0u;
  if (out_bytes == 1) launch_dtype<uint8_t>(dt, a, ctx->stream);
  else launch_dtype<uint16_t>(dt, a, ctx->stream);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  return SMESH_OK;
}

extern "C" int smesh_labels_prepare(const void* in, int label_dtype, const int64_t in_strides[2], int in_memkind, uint64_t w, uint64_t h,
                                    const int32_t* map, uint64_t map_len, int map_memkind, uint32_t C, void* out, int out_dtype, uint64_t W,
                                    uint64_t H, int device) {
  const LabelPrep p{w, h, map, map_len, map_memkind};
  SMESH_TRY(smesh_label_prep_check(label_dtype, in_strides, in_memkind, p, W, H, C));
  if (out_dtype != SMESH_LBL_U8 && out_dtype != SMESH_LBL_U16) return fail(SMESH_ERR_INVALID, "a prepared plane is uint8 or uint16");
  if (C == 0 || (out_dtype == SMESH_LBL_U8 && C > 255u)) return fail(SMESH_ERR_INVALID, "a uint8 plane holds 1 to 255 classes, a uint16 plane up to 65535");
  if (W == 0 || H == 0) return SMESH_OK;
  if (!in || !out) return fail(SMESH_ERR_INVALID, "NULL argument");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const int64_t dense[2] = {(int64_t)h, 1};
  const int64_t* s = in_strides ? in_strides : dense;
  const size_t span = ((1 + (w - 1) * (uint64_t)s[0] + (h - 1) * (uint64_t)s[1]) << (label_dtype >> 1));
  const size_t span_al = (span + 255) & ~(size_t)255;
  const bool stage_in = in_memkind == SMESH_MEM_HOST, stage_map = map && map_memkind == SMESH_MEM_HOST;
  char* tmp = nullptr;   // [the staged source][the staged map]
  if (stage_in || stage_map) SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&tmp), (stage_in ? span_al : 0) + (stage_map ? map_len * 4 : 0) + 256));
  int status = SMESH_OK;
  hipError_t e = hipSuccess;
  if (stage_in) {
    e = hipMemcpyAsync(tmp, in, span, hipMemcpyHostToDevice, ctx->stream);
    in = tmp;
  }
  if (e == hipSuccess && stage_map) {
    char* d = tmp + (stage_in ? span_al : 0);
    e = hipMemcpyAsync(d, map, map_len * 4, hipMemcpyHostToDevice, ctx->stream);
    map = reinterpret_cast<const int32_t*>(d);
  }
  if (e == hipSuccess) status = smesh_label_prep_launch(ctx, in, label_dtype, s, w, h, map, map_len, C, out, out_dtype == SMESH_LBL_U8 ? 1 : 2, W, H);
  if (e == hipSuccess && status == SMESH_OK) e = hipStreamSynchronize(ctx->stream);
  if (tmp) (void)dev_free(tmp);
  SMESH_HIP(e);
  return status;
}
