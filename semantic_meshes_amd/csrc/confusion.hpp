// confusion.hpp -- what the kernels that count into a confusion matrix share: eval.hip (k_confusion: labels and index images against
// ground truth, include/smesh_eval.h) and probs_labels.hip (k_probs_labels: a class-vector image arg-maxed and counted in one pass,
// include/smesh_probs_labels.h).  The matrix handle, the workgroup histogram's constants, how a ground-truth element becomes a class,
// how a wave adds its keys, and the host-side checks and staging of (W,H) images.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/smesh_eval.h"

struct smesh_confusion {
  smesh::DeviceCtx* ctx = nullptr;
  uint32_t C = 0;
  uint64_t nbins = 0;                       // C (C + 1)
  unsigned long long* d_counts = nullptr;   // [nbins + 1]: the matrix, then `ignored`
  std::vector<uint64_t> merged;             // smesh_confusion_add_counts: [nbins + 1] on the host, added by get(); empty until used
  smesh::Scratch stage_src, stage_gt, stage_lbl;   // device copies of HOST inputs (consumed before the call that staged them returns)
  std::mutex mu;                            // held for a whole entry point; taken before the renderer's and the context's locks
};

namespace smesh {

constexpr int kWave = 64;
// LDS budget of the histogram: 128 KiB of the CU's 160 KiB, declared statically.  Everything over 80 KiB means one workgroup per CU
// anyway, and C = 150 (90.6 KB) is well inside; the small instance (16 KiB: up to 63 classes, which covers 19 and 40) lets two
// workgroups share a CU.  kConfusionLdsMaxC (common.hpp) is the largest C with C (C + 1) + 1 counters in the budget.
constexpr uint32_t kLdsWordsSmall = 4096, kLdsWordsLarge = 32768;
static_assert((uint64_t)kConfusionLdsMaxC * (kConfusionLdsMaxC + 1) + 1 <= kLdsWordsLarge &&
              (uint64_t)(kConfusionLdsMaxC + 1) * (kConfusionLdsMaxC + 2) + 1 > kLdsWordsLarge, "kConfusionLdsMaxC does not match the LDS budget");
// In-wave aggregation: the lanes that share the first pending lane's key add their population count once.  Label images are large
// uniform regions -- one to three distinct keys per wave -- so after kAggRounds rounds whoever is left adds 1 for itself: a wave of
// 64 different keys pays three ballots, not 64.
constexpr int kAggRounds = 3;
constexpr uint32_t kNoClass = 0xFFFFFFFFu;

// A ground-truth element as a class, in two halves: the element's bits (one load, nothing computed from it: a kernel may keep it in
// flight), and its class -- its value where that lies in [0, C), else kNoClass (a negative value sign-extends to a huge one).  The
// width and the sign are read off the dtype code: the signed dtypes are the odd SMESH_LBL_* codes.
static_assert(SMESH_LBL_U8 == 0 && SMESH_LBL_I8 == 1 && SMESH_LBL_U16 == 2 && SMESH_LBL_I16 == 3 && SMESH_LBL_U32 == 4 && SMESH_LBL_I32 == 5 &&
              SMESH_LBL_U64 == 6 && SMESH_LBL_I64 == 7, "load_gt_bits / class_of_bits read the width and the sign off the dtype code");
__device__ __forceinline__ uint64_t load_gt_bits(const void* p, int dt, uint64_t off) {
  switch (dt >> 1) {
    case 0:  return static_cast<const uint8_t*>(p)[off];
    case 1:  return static_cast<const uint16_t*>(p)[off];
    case 2:  return static_cast<const uint32_t*>(p)[off];
    default: return static_cast<const uint64_t*>(p)[off];
  }
}
__device__ __forceinline__ uint32_t class_of_bits(uint64_t u, int dt, uint32_t C) {
  if (dt & 1) {
    const int sh = 64 - (8 << (dt >> 1));
    u = (uint64_t)((int64_t)(u << sh) >> sh);
  }
  return u < (uint64_t)C ? (uint32_t)u : kNoClass;
}
__device__ __forceinline__ uint32_t load_class(const void* p, int dt, uint64_t off, uint32_t C) {
  return class_of_bits(load_gt_bits(p, dt, off), dt, C);
}

template <bool IN_LDS>
__device__ __forceinline__ void add_count(uint32_t* hist, unsigned long long* counts, uint32_t key, uint32_t cnt) {
  if (IN_LDS) atomicAdd(&hist[key], cnt);
  else atomicAdd(&counts[key], (unsigned long long)cnt);
}

// One sample per lane (`on`: this lane has one).  Every lane of the wave gets here together.
template <bool IN_LDS>
__device__ __forceinline__ void add_keys(uint32_t* hist, unsigned long long* counts, uint32_t key, bool on, int aggregate) {
  if (aggregate) {
    const int lane = (int)(threadIdx.x & (kWave - 1));
    unsigned long long todo = __ballot(on);
    for (int round = 0; round < kAggRounds && todo; round++) {
      const int src = __ffsll((long long)todo) - 1;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, src);   // wave-uniform
      const bool mine = on && key == k;
      const unsigned long long same = __ballot(mine);
      if (lane == src) add_count<IN_LDS>(hist, counts, k, (uint32_t)__popcll(same));
      on = on && !mine;
      todo &= ~same;
    }
  }
  if (on) add_count<IN_LDS>(hist, counts, key, 1u);
}

inline size_t label_itemsize(int dt) { return (size_t)1 << (dt >> 1); }

inline bool bad_mem(int m) { return m != SMESH_MEM_HOST && m != SMESH_MEM_DEVICE; }

inline int check_image_size(uint64_t W, uint64_t H) {
  if (W > 65536 || H > 65536 || W * H >= 0x7FFFFFFFull / 4) return fail(SMESH_ERR_INVALID, "image too large");
  return SMESH_OK;
}

inline int check_gt(const void* gt, int dt, const int64_t* strides, int mem) {
  if (!gt) return fail(SMESH_ERR_INVALID, "NULL ground truth");
  if (dt < 0 || dt > SMESH_LBL_I64) return fail(SMESH_ERR_INVALID, "bad ground-truth dtype");
  if (strides && (strides[0] < 0 || strides[1] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (bad_mem(mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  return SMESH_OK;
}

inline bool is_dense(const int64_t* s, uint64_t W, uint64_t H) { return !s || ((s[0] == (int64_t)H || W == 1) && (s[1] == 1 || H == 1)); }

// A (W,H) image of `itemsize`-byte elements on the device: itself, or a copy of the span its strides cover in `stage`.
inline int image_on_device(DeviceCtx* ctx, Scratch& stage, const void* img, size_t itemsize, const int64_t* strides, int mem, uint64_t W, uint64_t H,
                           const void** out, bool* staged) {
  *out = img;
  if (mem == SMESH_MEM_DEVICE) return SMESH_OK;
  const int64_t dense[2] = {(int64_t)H, 1};
  const int64_t* s = strides ? strides : dense;
  const size_t span = (size_t)(1 + (W - 1) * (uint64_t)s[0] + (H - 1) * (uint64_t)s[1]) * itemsize;
  SMESH_TRY(stage.reserve(std::max<size_t>(span, 16)));
  SMESH_HIP(hipMemcpyAsync(stage.ptr, img, span, hipMemcpyHostToDevice, ctx->stream));
  *out = stage.ptr;
  *staged = true;
  return SMESH_OK;
}

}  // namespace smesh

// eval.hip: k_confusion in its labels mode over a DENSE int32 (W,H) label image on the device (y fastest) against a ground-truth
// image that is already on the device -- the second pass of smesh_confusion_add_probs for class counts beyond the single-pass
// kernel.  `cm` and its context locked, device current.
int smesh_confusion_count_label_image(smesh_confusion* cm, const int32_t* d_labels, const void* d_gt, int gt_dtype, const int64_t* gt_strides,
                                      uint64_t W, uint64_t H);
