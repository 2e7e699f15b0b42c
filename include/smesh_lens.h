/*
 * smesh_lens.h -- images from cameras with lens distortion, undistorted on the device: an extension of the C ABI in smesh.h.
 *
 * Every fusion call of smesh.h assumes a pinhole camera.  COLMAP's default model for a fresh reconstruction is SIMPLE_RADIAL; the
 * reference has its users run `colmap image_undistorter` first (eval-scannet/run_colmap_on_scannet.py:108, README: "send all
 * undistorted images through your segmentation model"), which writes a second copy of every image and puts the network on resampled
 * pixels.  The entry points below take an image on the SENSOR's grid -- class vectors, masks, colour masks, sensor depth, at any
 * size -- and give the image of the pinhole VIEW that is rendered: the forward model from ideal to distorted coordinates is closed
 * form for COLMAP's polynomial models, so a pixel of the view needs no iteration.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header; tests feed the oracle the numpy restatement
 * of the rule below (tests/lens_ref.py).
 *
 * The rule.  Inputs: a lens (smesh_lens_t: f, c, k1..k6, p1, p2 and the calibration size (wc, hc)), the view (the
 * F, P and (W, H) of a smesh_camera_t; its pose is not looked at) and a source image of (w, h) pixels, which need not be (wc, hc):
 * the network's resolution is served by the same rule.  For output pixel (X, Y), in IEEE double, every operation rounded
 * separately (no fma), in this order:
 *       x  = ((X + 0.5) - Px) / Fx          y likewise                      (the renderer's pixel centres)
 *       xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy
 *       n  = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *       d  = 1 + r2*(k4 + r2*(k5 + r2*k6))
 *       s  = n / d                          (k4 = k5 = k6 = 0: d is exactly 1 and the division is skipped, same bits)
 *       dx = (2*p1)*xy + p2*(r2 + 2*xx)     dy = p1*(r2 + 2*yy) + (2*p2)*xy
 *       xd = x*s + dx;  yd = y*s + dy
 *       u  = fx*xd + cx;  v = fy*yd + cy    (calibration pixels, pixel centres at +0.5: COLMAP's convention)
 *       tx = u*(w/wc) - 0.5;  ty = v*(h/hc) - 0.5                           (the two ratios divided on the host, in double)
 *       inside = d > 0 && -0.5 <= tx && tx <= w - 0.5 && -0.5 <= ty && ty <= h - 0.5         (a NaN is outside)
 * This is COLMAP's FULL_OPENCV.  OPENCV is k3 .. k6 = 0, RADIAL also p = 0, SIMPLE_RADIAL also k2 = 0.  The fisheye, FOV and
 * thin-prism models need atan, which cannot be pinned to the bit: they are not served.
 *   BILINEAR (class vectors): per axis t = min(max(t, 0), n - 1); i0 = floor(t); i1 = min(i0 + 1, n - 1); f = (float)(t - i0); then
 * the float32 blend of smesh_resize.h, unchanged; float16 / bfloat16 are widened exactly and a 16-bit output is narrowed by the
 * rule of smesh_narrow_probs.
 *   NEAREST (everything that must not be blended): per axis i = floor(t + 0.5), clamped to [0, n - 1].
 *   OUTSIDE pixels: a class-vector row is all +0.0f; a nearest pixel gets the caller's fill; the weights plane is
 * inside ? w_in : 0 with w_in the caller's (W,H) plane or 1.0f; `counts` are uint64 [pixels, outside].
 *
 * Two limits of the model, stated and not fixed in code:
 *   - The polynomial folds back beyond the radius it was calibrated for: r * s(r) stops growing, and a view camera much wider than
 *     the lens then samples folded-back pixels that still look valid (inside, weight 1).
 *   - The default view camera (data.LensCamera) has the lens's own f, c and size, like OpenCV's undistort with newCameraMatrix =
 *     cameraMatrix.  For a sane calibration that view stays inside the calibrated radius.
 *
 * Conventions are those of smesh_resize.h: class-vector images are (w,h,C), pixel images (w,h[,channels]); strides are in ELEMENTS
 * and >= 0, NULL means dense (last axis fastest); outputs are dense DEVICE arrays, (W,H,C) and (W,H[,channels]); every function
 * returns a status; SMESH_ERR_INVALID comes with a message (smesh_last_error) and leaves nothing changed.  Refused: NULL arguments, a
 * bad dtype, element size or channel count, negative strides, an empty source or calibration size, w, h, W, H > 65536 or W * H >=
 * 2^29, a lens or view parameter that is not finite, focal lengths not > 0, an output that overlaps the input.  W == 0 or H == 0:
 * nothing to do, counts [0, 0].
 *
 * Memory and order.  A HOST source is staged at the span its strides cover and consumed before the call returns; DEVICE arrays are
 * read and written asynchronously on the library's main stream and must stay valid until smesh_synchronize.  `counts` is HOST
 * memory: a call that asks for them waits for them.
 *
 * Paths.  smesh_undistort_probs takes the VECTOR path under the conditions of smesh_resize_probs: a lane owns 16 bytes of one
 * pixel's output row; a workgroup first computes the map of its run of pixels, one lane per pixel, into LDS, then blends.  Anything
 * else takes the GENERIC path, one lane per output element.  smesh_set_option("lens_vector", 0 | 1) (default 1) is a test hook: 0
 * sends every image down the generic path; results are the same.  smesh_get_option("lens_launches"): this process's launches of the
 * kernels of this header (read-only); smesh_get_option("last_lens_path"): the calling thread's last launch -- 0 none yet, 1 the
 * VECTOR path, 2 the GENERIC path, 3 the nearest kernel (read-only).  These entry points use no smesh_profile_* slot.
 */
#ifndef SMESH_LENS_H
#define SMESH_LENS_H

#include "smesh.h"
#include "smesh_half.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A polynomial lens: COLMAP's FULL_OPENCV parameters and the image size they were calibrated at. */
typedef struct smesh_lens_t {
  double focal[2];      /* fx, fy */
  double principal[2];  /* cx, cy */
  double k[6];          /* k1 .. k6 */
  double p[2];          /* p1, p2 */
  uint64_t width, height;
} smesh_lens_t;

/* The dense (W,H,C) class-vector image of `view`, (W,H) = (view->width, view->height), from the (w,h,C) image `in` on the sensor's
 * grid.  `weights_out_or_null`: a DEVICE (W,H) float32 plane that gets inside ? w_in : 0, from the same launch;
 * `weights_in_or_null`: a dense DEVICE (W,H) float32 plane (NULL: 1.0f).  `counts_or_null`: HOST uint64 [pixels, outside]. */
int smesh_undistort_probs(const void* in, int in_dtype, const int64_t in_strides[3], int in_memkind,
                          uint64_t w, uint64_t h, uint32_t C, const smesh_lens_t* lens, const smesh_camera_t* view,
                          void* out, int out_dtype, const float* weights_in_or_null, float* weights_out_or_null,
                          uint64_t* counts_or_null, int device);

/* The dense (W,H[,channels]) image of `view` from the (w,h[,channels]) image `in`, sampled nearest: pixels of `channels` (1 .. 4)
 * elements of `elem_bytes` (1, 2, 4 or 8) bytes -- masks of every integer dtype, colour masks, uint16 / float32 sensor depth.
 * `in_strides`: three element strides (the third is not looked at for one channel).  `fill`: HOST, `channels` elements, the pixel an
 * outside pixel gets. */
int smesh_undistort_pixels(const void* in, int elem_bytes, int channels, const int64_t in_strides[3], int in_memkind,
                           uint64_t w, uint64_t h, const smesh_lens_t* lens, const smesh_camera_t* view,
                           const void* fill, void* out, uint64_t* counts_or_null, int device);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_LENS_H */
