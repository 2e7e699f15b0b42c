// half_scratch.hpp -- what the 16-bit and sampled class-vector entry points (fusion_half.hip, fusion_sampled.hip) share with the rest
// of the library: the aggregator-owned device scratch (allocated on first use, released by smesh_aggregator_destroy, like
// LabelScratch), the staging of a group of host images into it, and the exact 16-bit conversions.
#pragma once

#include <mutex>

#include "common.hpp"
#include "view_input.hpp"

namespace smesh {

// Largest class count k_fuse_tri_h16 serves: run-time class counts in 8 / 16 .. 48 register slots, as k_fuse_tri's run-time-C
// instances.  Read-only option "half_max_classes" (smesh_get_option).
constexpr uint32_t kHalfMaxClasses = 48;

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

// Two packed elements -> two float32, exactly.  binary16: v_cvt_f32_f16 (the kernels run in hipcc's default mode, which keeps
// binary16 subnormals); bfloat16: the bits moved up.  (fusion_half.hip and probs_labels.hip widen with this and nothing else.)
__device__ __forceinline__ void unpack2(uint32_t w, bool bf, float& lo, float& hi) {
  if (bf) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xFFFF0000u);
  } else {
    const h16x2 h = __builtin_bit_cast(h16x2, w);
    lo = (float)h.x;
    hi = (float)h.y;
  }
}

// The narrowing of smesh_narrow_probs (fusion_half.hip; resize.hip rounds its 16-bit outputs with it).
// float32 -> bfloat16 bits, round to nearest even; NaN stays a (quiet) NaN, overflow rounds to inf.
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// float32 -> binary16 bits: v_cvt_f16_f32 in the default mode (round to nearest even, subnormal results kept, overflow to inf).
__device__ __forceinline__ uint32_t f16_rne(float x) {
  const _Float16 h = (_Float16)x;
  return (uint32_t)__builtin_bit_cast(uint16_t, h);
}

// Staged host images (16 bits per element) and staged weights of up to eight views, and the widened float32 image of the routes
// k_fuse_tri_h16 does not serve.  Everything that writes or reads them is ordered on the context's main stream.  `mu` is held for a
// whole entry point of smesh_half.h: it is taken before any other lock of the library, and by those entry points only.
// smp_*: the same for the entry points of smesh_sampled.h -- source images staged at their own size, staged weights, and the
// resampled (W,H,C) images of the views the sampling kernel does not serve.  `smp_mu` is held for a whole entry point of that header
// and taken before `mu` (those entry points call the ones of smesh_half.h).
struct HalfScratch {
  std::mutex mu, smp_mu;
  Scratch stage, w, wide;
  Scratch smp_stage, smp_w, smp_full;
  void release() { stage.release(); w.release(); wide.release(); smp_stage.release(); smp_w.release(); smp_full.release(); }
};

// The host images and host weights of a group of m <= kGroup views into reserved scratch, on the main stream, and the wait for the
// copies (the caller may reuse its host arrays once its call returns).  `stage` (null: the images stay where they are): image v, of
// image_bytes(v) bytes, goes to slot v, the slots slot_bytes apart; `w`: the same for the (W,H) float32 weights of the views that have
// some.  dev[v] / wts[v]: where view v's image and weights are now.  The context is locked and its device current.
template <typename ImageBytes>
int stage_host_group(DeviceCtx* ctx, const smesh_camera_t* cams, int m, const void* const* probs, const float* const* weights, Scratch* stage,
                     size_t slot_bytes, ImageBytes image_bytes, Scratch& w, size_t w_bytes, const void** dev, const float** wts) {
  for (int v = 0; v < m; v++) {
    dev[v] = probs[v];
    wts[v] = weights ? weights[v] : nullptr;
    if (stage) {
      char* d = static_cast<char*>(stage->ptr) + (size_t)v * slot_bytes;
      SMESH_HIP(hipMemcpyAsync(d, probs[v], image_bytes(v), hipMemcpyHostToDevice, ctx->stream));
      dev[v] = d;
    }
    if (wts[v]) {
      float* dw = reinterpret_cast<float*>(static_cast<char*>(w.ptr) + (size_t)v * w_bytes);
      SMESH_HIP(hipMemcpyAsync(dw, wts[v], cams[v].width * cams[v].height * 4, hipMemcpyHostToDevice, ctx->stream));
      wts[v] = dw;
    }
  }
  SMESH_HIP(hipStreamSynchronize(ctx->stream));
  return SMESH_OK;
}

}  // namespace smesh
