// view_input.hpp -- what a view's image IS on its way from an entry point (fusion.hip's float32 class vectors, fusion_labels.hip,
// fusion_half.hip, fusion_sampled.hip) through raster.hip's view drivers to the fusion kernel that reads it, and the few constants
// that the entry points staging groups of host images share.
#pragma once

#include <cstddef>
#include <cstdint>

namespace smesh {

// (w,h,C) class vectors at the network's resolution, sampled inside the fusion kernel (fusion_sampled.hip, include/smesh_sampled.h).
struct SampledSrc {
  int dtype;          // SMESH_PROBS_* of every image of the call
  uint32_t w, h;      // their width and height
  int64_t s0, s1;     // element strides of x and y (class stride 1)
};

// One view's image.  HOST memory only for F32 (the drivers stage it); every other kind is in DEVICE memory.
struct ViewInput {
  enum Kind {
    F32,       // float32 class vectors (W,H,C); ps0 / ps1: element strides of x and y where not dense (0, 0: dense)
    LABELS,    // a dense (W,H) label plane, `dtype_or_bytes` = 1 or 2 bytes per label (k_fuse_tri_labels, or expanded to F32)
    HALF,      // float16 / bfloat16 class vectors (W,H,C), `dtype_or_bytes` = SMESH_PROBS_*, class stride 1, ps0 / ps1 as F32
               // (k_fuse_tri_h16, or widened to F32)
    SAMPLED,   // a (w,h,C) image that `src` describes (k_fuse_tri_sampled; the caller made sure that kernel serves the call)
  } kind = F32;
  int dtype_or_bytes = 0;
  const void* image = nullptr;
  int64_t ps0 = 0, ps1 = 0;
  SampledSrc src{};

  static ViewInput f32(const float* probs, int64_t ps0 = 0, int64_t ps1 = 0) { return ViewInput{F32, 0, probs, ps0, ps1}; }
  static ViewInput labels(const void* plane, int bytes) { return ViewInput{LABELS, bytes, plane}; }
  static ViewInput half(const void* image, int dtype, int64_t ps0 = 0, int64_t ps1 = 0) { return ViewInput{HALF, dtype, image, ps0, ps1}; }
  static ViewInput sampled(const void* image, const SampledSrc& src) { return ViewInput{SAMPLED, src.dtype, image, 0, 0, src}; }
  // The same kind of input, another view's image (a call's views share everything else).
  ViewInput at(const void* other) const { ViewInput v = *this; v.image = other; return v; }
  const float* probs() const { return kind == F32 ? static_cast<const float*>(image) : nullptr; }
};

constexpr int kGroup = 8;   // views whose staged or prepared images share an aggregator's scratch: a group of smesh_fuse_views

inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// Elements that the strides `s` of a (w,h,C) image cover.
inline uint64_t source_span(const int64_t* s, uint64_t w, uint64_t h, uint32_t C) {
  return 1 + (w - 1) * (uint64_t)s[0] + (h - 1) * (uint64_t)s[1] + (uint64_t)(C - 1) * (uint64_t)s[2];
}

}  // namespace smesh
