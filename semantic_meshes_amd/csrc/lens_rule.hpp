// lens_rule.hpp -- the undistortion rule of include/smesh_lens.h, written once on the device side: lens.hip maps
// every pixel of the pinhole view to the source image with it.  IEEE double, every operation rounded separately (the library is
// built with -ffp-contract=off), in the order the header states.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "resize_rule.hpp"

namespace smesh {

// The lens, the view and the source size, as the kernels take them.
struct LensMap {
  double Fx, Fy, Px, Py;        // the pinhole view that is rendered
  double fx, fy, cx, cy;        // the lens
  double k1, k2, k3, k4, k5, k6;
  double p1x2, p2x2, p1, p2;    // 2 p is exact: doubled on the host
  double rx, ry;                // (double)w / (double)wc and (double)h / (double)hc, divided on the host
  double xmax, ymax;            // w - 0.5 and h - 0.5
  uint32_t w, h;                // the source image
  uint32_t rational;            // any of k4 .. k6 is not zero: d is not exactly 1
};

// Where output pixel (X, Y) lies in the source image, in its pixel coordinates (pixel centres at integers).
struct LensTap {
  double tx, ty;
  bool inside;
};
__device__ __forceinline__ LensTap lens_tap(const LensMap& m, uint32_t X, uint32_t Y) {
  const double x = (((double)X + 0.5) - m.Px) / m.Fx, y = (((double)Y + 0.5) - m.Py) / m.Fy;
  const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
  const double n = 1.0 + r2 * (m.k1 + r2 * (m.k2 + r2 * m.k3));
  double d = 1.0, s = n;
  if (m.rational) {             // (uniform over the launch)
    d = 1.0 + r2 * (m.k4 + r2 * (m.k5 + r2 * m.k6));
    s = n / d;
  }
  const double dx = m.p1x2 * xy + m.p2 * (r2 + 2.0 * xx), dy = m.p1 * (r2 + 2.0 * yy) + m.p2x2 * xy;
  const double xd = x * s + dx, yd = y * s + dy;
  const double u = m.fx * xd + m.cx, v = m.fy * yd + m.cy;
  LensTap t;
  t.tx = u * m.rx - 0.5;
  t.ty = v * m.ry - 0.5;
  t.inside = d > 0.0 && -0.5 <= t.tx && t.tx <= m.xmax && -0.5 <= t.ty && t.ty <= m.ymax;   // (a NaN is outside)
  return t;
}

// Bilinear: one axis of an INSIDE tap, clamped like axis_of() of resize_rule.hpp.
__device__ __forceinline__ Axis lens_axis(double t, uint32_t n) {
  t = fmin(fmax(t, 0.0), (double)(n - 1u));
  const double fl = floor(t);
  Axis a;
  a.i0 = (uint32_t)fl;
  a.i1 = a.i0 + 1u < n ? a.i0 + 1u : n - 1u;
  a.f = (float)(t - fl);
  return a;
}

// Nearest: one axis of an INSIDE tap.
__device__ __forceinline__ uint32_t lens_nearest(double t, uint32_t n) {
  const double i = fmin(fmax(floor(t + 0.5), 0.0), (double)(n - 1u));
  return (uint32_t)i;
}

}  // namespace smesh
