/*
 * smesh_probs_labels.h -- the labels of a class-vector image, and their confusion matrix, on the device: an extension of the C ABI
 * in smesh.h.
 *
 * The reference's evaluation (eval-scannet/eval_scannet.py:113-117, :232-236) scores the network's own prediction per pixel: each
 * frame's (H,W,C) class-vector image is arg-maxed and counted against the ground-truth label image -- the baseline that the fused
 * mesh is compared with.  The entry points below do that where the image is: one streaming read of the image, one label per pixel
 * out, and (smesh_confusion_add_probs) the counts of smesh_eval.h in the same pass.
 *
 * PRODUCT-ONLY: oracle/libsmesh_oracle.so implements smesh.h and nothing of this header.
 *
 * The rule.  The label of a class vector r[0 .. C) of float32 -- or of float16 / bfloat16 widened exactly as
 * smesh_half.h defines -- is
 *     best = r[0]; label = 0
 *     for c = 1 .. C-1 in ascending order: if (r[c] > best) { best = r[c]; label = c }
 * so: the lowest class among equals; a NaN element never replaces the current best; a NaN r[0] is never replaced; +0 and -0 are
 * equal; rows need not be probabilities (negative values and infinities are ordinary values).
 * The optional don't-care test is the rule of smesh_eval.h for an aggregator row: t = the float32 sum of r[c] in ascending class
 * order, starting from 0.0f; the pixel is DON'T CARE iff t < dont_care_threshold (false for a NaN t).  dont_care_threshold =
 * -INFINITY means "no test": no sum is computed and every pixel gets a label.
 *
 * Conventions are those of smesh_half.h and smesh_labels.h: class-vector images are (W,H,C), label and ground-truth images (W,H);
 * strides are in ELEMENTS and >= 0, NULL means dense (class fastest, then y); `probs_dtype` is SMESH_PROBS_F32 | F16 | BF16; every
 * function returns a status; SMESH_ERR_INVALID comes with a message (smesh_last_error) and leaves nothing changed -- neither the
 * output image nor the matrix.  Limits: W, H <= 65536 and W * H < 2^29; element offsets are 64-bit.  W == 0 or H == 0: nothing to do.
 *
 * Paths.  An image whose class stride is 1 and one of whose pixel axes has stride C (the dense (W,H,C) image: y; a network's
 * (H,W,C) tensor seen as (W,H,C): x) with C <= "probs_labels_tile_max_classes" (255; read-only, smesh_get_option) is read in TILES:
 * a workgroup loads consecutive pixels' rows as one contiguous span with 16-byte loads, stages them in LDS and scans one row per
 * lane.  Everything else -- other class strides, channel-first views, zero strides, more classes, runs shorter than 32 bytes -- takes
 * the GENERIC path: one lane per pixel, strided loads.  smesh_set_option("probs_labels_tiles", 0 | 1) (default 1) is a test hook:
 * 0 sends every image down the generic path; results are the same.  smesh_confusion_add_probs labels and counts in ONE kernel up to
 * 63 classes (the small LDS histogram of smesh_eval.h); beyond that the labels go as int32 into library scratch and k_confusion
 * counts them (two launches).  Read-only, reporting (smesh_get_option): "last_probs_labels_grid" is the number of workgroups of the
 * calling thread's last launch of either path, "last_probs_labels_work" what they shared out -- tiles on the tiled path, rounds of
 * 256 pixels on the generic one; a launch with work > grid had workgroups that took more than one.  Both are 0 before the first launch.
 */
#ifndef SMESH_PROBS_LABELS_H
#define SMESH_PROBS_LABELS_H

#include "smesh.h"
#include "smesh_labels.h"
#include "smesh_half.h"
#include "smesh_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* smesh_profile_* slot of the labelling kernel: the LAST free slot of SMESH_PROF_SLOTS (8) -- 5 is smesh_eval.h's, 6
 * smesh_label_images.h's.  Both entry points bracket their kernel with it. */
#define SMESH_PROF_PROBS_LABELS 7

/* out[x, y] = the label of probs[x, y, :], or `dont_care_value` for a don't-care pixel.  `out_dtype`: SMESH_LBL_U8 (C <= 255),
 * SMESH_LBL_U16 (C <= 65535) or SMESH_LBL_I32; a dtype too narrow for C, a `dont_care_value` inside [0, C) or one that `out_dtype`
 * cannot hold is refused.  Asynchronous for DEVICE arrays (they must stay valid until smesh_synchronize); a HOST image is staged at
 * its own width (a 16-bit image crosses PCIe at 16 bits) and a call with a HOST array returns when `out` is complete. */
int smesh_probs_labels(const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_memkind,
                       uint64_t W, uint64_t H, uint32_t C, float dont_care_threshold,
                       void* out, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value, int out_memkind, int device);

/* Counts M[gt, label] by the definitions of smesh_eval.h: a don't-care prediction goes to column C, ground truth outside [0, C)
 * to `ignored`.  The class count is the matrix's.  `labels_out_or_null`: a DEVICE (W,H) image of `out_dtype` / `out_strides` /
 * `dont_care_value` (as above) that the same pass writes; NULL: the three arguments are not looked at.  HOST inputs are consumed
 * before the call returns; DEVICE arrays must stay valid until smesh_synchronize or smesh_confusion_get. */
int smesh_confusion_add_probs(smesh_confusion_t* cm,
                              const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_memkind,
                              const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_memkind,
                              uint64_t W, uint64_t H, float dont_care_threshold,
                              void* labels_out_or_null, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value);

#ifdef __cplusplus
}
#endif

#endif /* SMESH_PROBS_LABELS_H */
