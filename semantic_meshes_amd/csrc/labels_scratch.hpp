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
  Scratch map;   // the staged host map of a prepared call (smesh_label_prep.h)
  void release() { stage.release(); plane.release(); w.release(); onehot.release(); map.release(); }
};

// What the prepared entry points (smesh_label_prep.h) add to their smesh_labels.h counterparts: the label images are (w,h), and their
// values go through `map` (int32 [map_len] in `map_mem` memory; NULL: none).
// Colour images (smesh_label_colors.h): `channels` 3 or 4 (0: a plain label image) -- the images are uint8 (w,h,channels) with a third
// stride, there is no map, and their keys go through the table (`keys`, `classes`: HOST memory, `table_len` pairs).
struct LabelPrep {
  uint64_t w, h;
  const int32_t* map;
  uint64_t map_len;
  int map_mem;
  int channels = 0;
  const uint32_t* keys = nullptr;
  const int32_t* classes = nullptr;
  uint64_t table_len = 0;
};

// A call's map or colour table in device memory (fusion_labels.hip stage_map): `map` is the map, or the table's classes beside `keys`.
struct LabelTableDev {
  const int32_t* map = nullptr;
  const uint32_t* keys = nullptr;
};

}  // namespace smesh

// label_colors.hip.  smesh_label_colors_check: the refusals of smesh_label_colors.h that concern the image's format and the table
// (the sizes are smesh_label_prep_check's).  smesh_label_colors_launch: k_labels_prepare_colors on the context's main stream -- `src`,
// `keys_dev` and `classes_dev` in device memory, `strides` three element strides, `out` the dense (W,H) plane of `out_bytes` (1 or 2)
// bytes per pixel; the caller has checked the arguments and holds the context's lock.
int smesh_label_colors_check(int label_dtype, const int64_t* strides, const smesh::LabelPrep& p);
int smesh_label_colors_launch(smesh::DeviceCtx* ctx, const void* src, const int64_t* strides, uint64_t w, uint64_t h, const uint32_t* keys_dev,
                              const int32_t* classes_dev, uint64_t K, uint32_t C, void* out, int out_bytes, uint64_t W, uint64_t H);

// label_prep.hip.  smesh_label_prep_check: the refusals of smesh_label_prep.h for one (w,h) -> (W,H) pair.  smesh_label_prep_launch:
// k_labels_prepare on the context's main stream -- `src` and `map_dev` in device memory, `out` the dense (W,H) plane of `out_bytes`
// (1 or 2) bytes per pixel; the caller has checked the arguments and holds the context's lock.
int smesh_label_prep_check(int label_dtype, const int64_t* strides, int memkind, const smesh::LabelPrep& p, uint64_t W, uint64_t H, uint32_t C);
int smesh_label_prep_launch(smesh::DeviceCtx* ctx, const void* src, int label_dtype, const int64_t* strides, uint64_t w, uint64_t h,
                            const int32_t* map_dev, uint64_t map_len, uint32_t C, void* out, int out_bytes, uint64_t W, uint64_t H);
