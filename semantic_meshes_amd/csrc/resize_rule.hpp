// resize_rule.hpp -- the resampling rule of include/smesh_resize.h, written once: resize.hip builds images with it,
// fusion_sampled.hip samples a pixel's class vector with it inside the fusion kernel.  The source coordinates in double, the three
// lerps in float32, every operation rounded separately (the library is built with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace smesh {

// One axis of the rule: output coordinate X of N, input size n, s = (double)n / (double)N.
struct Axis {
  uint32_t i0, i1;
  float f;
};
__device__ __forceinline__ Axis axis_of(uint32_t X, double s, uint32_t n) {
  double t = ((double)X + 0.5) * s - 0.5;
  t = fmin(fmax(t, 0.0), (double)(n - 1u));
  const double fl = floor(t);
  Axis a;
  a.i0 = (uint32_t)fl;                                  // in [0, n - 1]: t is clamped
  a.i1 = a.i0 + 1u < n ? a.i0 + 1u : n - 1u;
  a.f = (float)(t - fl);
  return a;
}

__device__ __forceinline__ float lerp1(float a, float b, float f) { return f == 0.0f ? a : a + (b - a) * f; }
__device__ __forceinline__ float blend(float a00, float a10, float a01, float a11, float fx, float fy) {
  return lerp1(lerp1(a00, a10, fx), lerp1(a01, a11, fx), fy);
}

}  // namespace smesh
