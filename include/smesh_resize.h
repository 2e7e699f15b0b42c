/*
 * smesh_resize.h -- class-vector images at the network's resolution, resampled to the camera's on the device: an extension of the C
 * ABI in smesh.h.
 *
 * A segmentation network rarely runs at the camera's resolution.  The reference's evaluation (eval-scannet/eval_scannet.py:221-236)
 * resizes the (480,640,40) prediction to (968,1296,40) in its framework before it scores and fuses it; every entry point of smesh.h
 * refuses an image whose width and height are not the index plane's.  The entry points below resample a (w,h,C) image to the dense
 * (W,H,C) image the fusion kernels read, label the resampled image without building it, and count those labels against ground truth.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header; tests feed the oracle the numpy restatement
 * of the rule below.
 *
 * The rule.  SMESH_RESIZE_BILINEAR is bilinear interpolation with half-pixel centres and no antialiasing -- what
 * tf.image.resize(..., "bilinear") of TF2 and torch.nn.functional.interpolate(mode="bilinear", align_corners=False) mean, up to
 * rounding -- defined to the bit:
 *   per axis (input size n, output size N, output coordinate X), in IEEE double, every operation rounded separately (no fma):
 *       s  = (double)n / (double)N
 *       t  = (X + 0.5) * s - 0.5
 *       t  = min(max(t, 0.0), (double)(n - 1))
 *       i0 = floor(t);  i1 = min(i0 + 1, n - 1);  f = (float)(t - i0)            (so f == 0 whenever i1 == i0)
 *   per element, in float32, every operation rounded separately:
 *       lerp(a, b, f) = (f == 0) ? a : a + (b - a) * f
 *       top = lerp(in[x0, y0, c], in[x1, y0, c], fx);  bot = lerp(in[x0, y1, c], in[x1, y1, c], fx)
 *       out[X, Y, c] = lerp(top, bot, fy)
 * float16 / bfloat16 elements are widened exactly first (smesh_half.h).  So: (W,H) == (w,h) is an exact copy, NaN and infinities
 * included; a constant image stays constant; downscaling is plain bilinear sampling, with aliasing.  A 16-bit `out_dtype` rounds the
 * float32 result by the rule of smesh_narrow_probs (nearest even, overflow to inf, subnormals kept).
 * The LABEL of a resampled pixel is the rule of smesh_probs_labels.h applied to the float32 row out[X, Y, :] BEFORE any narrowing:
 * the lowest class among the largest values, a NaN never replaces the best; the optional don't-care test is the ascending float32
 * sum from 0.0f against `dont_care_threshold` (-INFINITY: no test).
 *
 * Conventions are those of smesh_probs_labels.h: class-vector images are (w,h,C), label and ground-truth images (W,H); strides are
 * in ELEMENTS and >= 0, NULL means dense (class fastest, then y) -- a network's (h,w,C) tensor and a channel-first (C,h,w) tensor are
 * both valid as permuted views; `in_dtype` / `out_dtype` of a class-vector image are SMESH_PROBS_F32 | F16 | BF16; every function
 * returns a status; SMESH_ERR_INVALID comes with a message (smesh_last_error) and leaves nothing changed.  Limits: W, H, w, h <=
 * 65536 and W * H < 2^29; element offsets are 64-bit.  W == 0 or H == 0: nothing to do.  Refused: w == 0 or h == 0 with a non-empty
 * target, C == 0, a bad dtype or mode, an `out` range that overlaps `in`.
 *
 * Memory and order.  `out` is DEVICE memory.  A HOST input is staged at its own size and width (w h C elements cross PCIe) and is
 * consumed before the call returns; DEVICE arrays are read and written asynchronously on the library's main stream and must stay
 * valid until smesh_synchronize.
 *
 * Paths.  smesh_resize_probs takes the VECTOR path when the class stride is 1, C is a multiple of the 16 / sizeof(out element)
 * elements a lane owns, and the bases and pixel strides are aligned to a lane's loads and stores: four corner loads, a float32
 * blend, one 16-byte store per lane, lanes along the output's memory order.  Everything else takes the GENERIC path: one lane per
 * output element.  smesh_set_option("resize_vector", 0 | 1) (default 1) is a test hook: 0 sends every image down the generic path;
 * results are the same.  These entry points use no smesh_profile_* slot.
 */
#ifndef SMESH_RESIZE_H
#define SMESH_RESIZE_H

#include "smesh.h"
#include "smesh_labels.h"
#include "smesh_half.h"
#include "smesh_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- resampling modes ---------------------------------------------------------------------- */
#define SMESH_RESIZE_BILINEAR 1

/* out[X, Y, c] for the whole dense (W,H,C) image of `out_dtype`. */
int smesh_resize_probs(const void* in, int in_dtype, const int64_t in_strides[3], int in_memkind,
                       uint64_t w, uint64_t h, uint32_t C,
                       void* out, int out_dtype, uint64_t W, uint64_t H, int mode, int device);

/* out[X, Y] = the label of the resampled row, or `dont_care_value` for a don't-care pixel, without any (W,H,C) image being built.
 * `out`: a DEVICE (W,H) image of `out_dtype` -- SMESH_LBL_U8 (C <= 255), SMESH_LBL_U16 (C <= 65535) or SMESH_LBL_I32 -- and
 * `out_strides`; a dtype too narrow for C, a `dont_care_value` inside [0, C) or one that `out_dtype` cannot hold is refused. */
int smesh_resize_probs_labels(const void* in, int in_dtype, const int64_t in_strides[3], int in_memkind,
                              uint64_t w, uint64_t h, uint32_t C, float dont_care_threshold,
                              void* out, int out_dtype, const int64_t out_strides[2],
                              int64_t dont_care_value, uint64_t W, uint64_t H, int mode, int device);

/* smesh_confusion_add_probs (smesh_probs_labels.h) for a (w,h,C) image against (W,H) ground truth: the labels of the resampled
 * image go as int32 into library scratch and the counting kernel of smesh_eval.h counts them (two launches, whatever the class
 * count).  `labels_out_or_null`: a DEVICE (W,H) image that the labelling pass also writes; NULL: the three arguments after it are
 * not looked at.  HOST inputs are consumed before the call returns; DEVICE arrays must stay valid until smesh_synchronize or
 * smesh_confusion_get. */
int smesh_confusion_add_probs_resized(smesh_confusion_t* cm,
                                      const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_memkind,
                                      uint64_t w, uint64_t h,
                                      const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_memkind, uint64_t W, uint64_t H,
                                      float dont_care_threshold, int mode,
                                      void* labels_out_or_null, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_RESIZE_H */
