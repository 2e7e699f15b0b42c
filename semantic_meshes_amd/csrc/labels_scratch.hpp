// labels_scratch.hpp -- device scratch of the label entry points (fusion_labels.hip), owned by the aggregator like its other staging
// buffers (fusion.hip: allocated on first use, released by smesh_aggregator_destroy).
#pragma once

#include <mutex>

#include "common.hpp"

namespace smesh {

// Largest class count whose 64-row block the main waves of k_fuse_tri_labels keep in LDS: rows of C | 1 floats (odd in banks), 64 of
// them in at most 64 KiB -- what a workgroup gets without asking -- so 255 classes, which is also where the narrow plane turns from
// uint8 to uint16.  At 19 classes a wave holds 4.9 KB (32 waves per CU), at 150 38.7 KB (4 waves per CU).  Beyond, the owner lane
// read-modify-writes acc[p * C + label] in global memory: one owner per row, no atomics, the same order of additions; no speed is
// claimed for it.  Read-only option "labels_lds_max_classes" (smesh_get_option).
constexpr uint32_t kLabelsLdsMaxC = 255;

// Staged host images, the narrowed planes and staged weights of up to eight views, and the fallback's one-hot expansion.  Everything
// that writes or reads them is ordered on the context's main stream.  `mu` is held for a whole label entry point: it is taken before
// any other lock of the library, and by those entry points only.
struct LabelScratch {
  std::mutex mu;
  Scratch stage, plane, w, onehot;
  void release() { stage.release(); plane.release(); w.release(); onehot.release(); }
};

}  // namespace smesh
