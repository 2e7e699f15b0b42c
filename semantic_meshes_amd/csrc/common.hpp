// common.hpp -- shared host-side plumbing of libsmesh_hip.so (device contexts, errors, timing).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/smesh.h"
#include "records.hpp"

namespace smesh {

int fail(int code, const std::string& msg);
int fail_hip(hipError_t e, const char* what, const char* file, int line);

#define SMESH_HIP(expr)                                                         \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess) return ::smesh::fail_hip(_e, #expr, __FILE__, __LINE__); \
  } while (0)

#define SMESH_TRY(expr)              \
  do {                               \
    int _s = (expr);                 \
    if (_s != SMESH_OK) return _s;   \
  } while (0)

struct ProfSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;  // recorded, not yet read
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;     // free event pairs
  double total_ms = 0.0;
  uint64_t launches = 0;
  uint64_t seen = 0;   // regions entered while the slot was enabled (only every `profile_every`-th is bracketed)
  int depth = 0;       // > 0 inside a region of this slot: nested regions belong to it (back-to-back launches timed together)
  bool open_timed = false;   // the region that is open right now is one of the bracketed ones
  uint64_t timed_launches = 0;   // launches of the slot's dominant kernel inside bracketed regions (prof_note) ...
  uint64_t timed_views = 0;      // ... and the views those launches fused
};

// One per GPU: a compute stream all of this library's kernels and copies are ordered on.
struct DeviceCtx {
  int device = -1;
  hipStream_t stream = nullptr;         // main stream: fusion kernels, copies, everything by default
  hipStream_t raster_stream = nullptr;  // smesh_fuse_view rasterises view k+1 here while view k is being fused
  hipStream_t exchange_stream = nullptr;   // smesh_allreduce_rows: the collective of a finished row range runs here, beside the fusion of the next
  hipEvent_t ev_order = nullptr;        // smesh_stream_wait: marks the producer's stream
  hipEvent_t ev_release = nullptr;      // smesh_stream_release: marks the library's stream
  int num_cus = 256;
  uint32_t lds_per_cu = 65536;          // bytes of LDS a CU's workgroups share (gfx950: 163 840)
  unsigned profiling = 0;   // bit s set = bracket slot s with HIP events
  unsigned profile_every = 1;   // ... every n-th region of the slot (an event pair costs ~4 us of stream time)
  ProfSlot slots[SMESH_PROF_SLOTS];
  hipEvent_t marks[SMESH_STREAM_MARKS] = {};   // smesh_stream_mark
  std::vector<hipEvent_t> token_pool;          // smesh_token_record / _done: events waiting for their next use
  std::recursive_mutex mu;
};

// Returns the context of `device`, creating it (and its stream) on first use.
int get_ctx(int device, DeviceCtx** out);

// RAII: brackets a region of the context's stream with HIP events when profiling is enabled.
struct ProfScope {
  DeviceCtx* ctx;
  int slot;
  hipEvent_t start = nullptr, stop = nullptr;
  hipStream_t st;
  bool counted = false;   // this scope opened a region (as opposed to: profiling off, or nested in an open region)
  ProfScope(DeviceCtx* c, int s, hipStream_t stream = nullptr);
  ~ProfScope();
};

// Called where a slot's dominant kernel is launched: counts the launch and the views it processes if (and only if) it falls
// inside a region that is being timed, so that total_ms / timed_launches is that kernel's average duration whatever the
// grouping of views into calls was.
void prof_note(DeviceCtx* ctx, int slot, uint64_t launches, uint64_t views);

// Device memory of the library: hipMalloc / hipFree with a cache of still-mapped blocks in between (context.cpp: why).
// dev_malloc allocates on the CURRENT device; the contents of a block are unspecified; dev_free returns when the device is idle.
hipError_t dev_malloc(void** out, size_t bytes);
hipError_t dev_free(void* p, bool foreign = false);   // foreign: the caller could see the block -- wait for the whole device
uint64_t dev_cached_bytes(int device);
void dev_trim(int device);
void dev_cache_stats(uint64_t* live_blocks, uint64_t* cached_blocks, uint64_t* cached_bytes);

// Run-time options (smesh_set_option; the environment supplies the defaults).  group_pipeline: smesh_fuse_views rasterises group
// g + 1 on the raster stream beside the fusion of group g (default on; SMESH_GROUP_PIPELINE=0).
bool opt_group_pipeline();
// raster_meshlets: the grouped launches of the one-lane-per-triangle rasteriser instances read per-block vertex tables built once per
// renderer and run without a vertex stage (raster.hip: render_group_into; SMESH_RASTER_MESHLETS=0 / 1).
constexpr int kRasterMeshletsDefault = 1;
bool opt_raster_meshlets();
// compact_records (SMESH_COMPACT_RECORDS; default 1): the raster launches of smesh_fuse_view(s) whose records only k_fuse_tri reads
// (float32 class vectors, triangle renderer in the caller's face order, images of at most 8 192 x 8 192) leave 8-byte records
// (records.hpp); 0: every launch leaves TriFrag, kernel for kernel what the library did before.  Same results either way.
constexpr int kCompactRecordsDefault = 1;
bool opt_compact_records();
// packed_fragments (SMESH_PACKED_FRAGMENTS; default 1): the fragment queues of a triangle renderer of at most 2^22 faces hold one 8-byte
// entry per fragment (fragments.hpp) instead of a 64-bit key and a 16-bit pixel in two arrays; read per raster launch.  0, texel
// renderers and larger meshes: the 10-byte format, kernel for kernel what the library did before.  Same results either way.
constexpr int kPackedFragmentsDefault = 1;
bool opt_packed_fragments();
// pipeline_fit (SMESH_PIPELINE_FIT; default 1): the LDS pad that caps the eight-view fusion launch of the group pipeline is computed from
// the device's LDS and the instance's own (pipeline_fuse_pad below); 0: the constant 24 576 bytes of rounds 2 - 6, kept selectable so that
// both can be compared in one process.  Same results either way.
// pipeline_fuse_waves (SMESH_PIPELINE_FUSE_WAVES; default kPipelineFuseWaves): the fusion waves per CU the computed pad allows at most.
// pipeline_fuse_pad (SMESH_PIPELINE_FUSE_PAD; default -1: none): a pad in bytes that overrides both.
constexpr int kPipelineFitDefault = 1;
constexpr int kPipelineFuseWaves = 5;
int opt_pipeline_fit();
int opt_pipeline_fuse_waves();
int opt_pipeline_fuse_pad();

// What runs on the raster stream beside a pipelined fusion launch: the LDS and registers of a workgroup (four waves, one per SIMD) of
// the fragment kernel of the renderer at hand.  Zero: not known.
struct PipelineNeighbour {
  uint32_t wg_lds = 0, wg_vgprs = 0;
};

// The dynamic LDS of a one-wave fusion workgroup that lets `want` of them onto a CU and no more: the smallest such pad, which leaves
// the neighbour the most.  *beside (may be null): how many rasteriser workgroups then fit beside `want` fusion waves, by the LDS that
// is left and by the registers -- the SIMD with the most fusion waves decides, a workgroup puts a wave on each.  Registers are
// allocated in eights out of 512 per SIMD lane and a SIMD holds eight waves; LDS is counted in blocks of 1 280 bytes, a multiple of
// every allocation granule of the CDNA parts.  `static_lds`, `vgprs`: of the fusion instance.  (`want` is held between 2 and 32: half
// a CU's LDS is more than a launch may ask for.  Lowering `want` until all the workgroups the registers allow also fit the LDS was
// tried and lost: the fusion launch needs its five waves more than the rasteriser needs a third workgroup, NOTES/pipeline_fit.md.)
inline uint32_t pipeline_fuse_pad(uint32_t lds_per_cu, uint32_t static_lds, uint32_t vgprs, int want, const PipelineNeighbour& nb,
                                  int* beside = nullptr) {
  constexpr uint32_t kBlock = 1280u;
  auto blocks = [&](uint32_t bytes) { return (bytes + kBlock - 1u) / kBlock * kBlock; };
  const uint32_t n = (uint32_t)std::min(32, std::max(2, want));
  // the smallest workgroup, in whole blocks, of which n + 1 no longer fit
  const uint32_t wg = std::max(blocks(static_lds), (lds_per_cu / (n + 1u)) / kBlock * kBlock + kBlock);
  if (beside) {
    const uint32_t alloc_f = std::max(8u, (vgprs + 7u) / 8u * 8u), alloc_r = std::max(8u, (nb.wg_vgprs + 7u) / 8u * 8u);
    const uint32_t per_simd = (n + 3u) / 4u;
    const uint32_t left = (uint64_t)wg * n <= lds_per_cu ? lds_per_cu - wg * n : 0u;
    const uint32_t regs_left = per_simd * alloc_f < 512u ? 512u - per_simd * alloc_f : 0u;
    const uint32_t by_regs = std::min(regs_left / alloc_r, per_simd < 8u ? 8u - per_simd : 0u);
    *beside = (int)std::min(by_regs, nb.wg_lds ? left / blocks(nb.wg_lds) : by_regs);
  }
  return wg - static_lds;
}
// confusion_wave_aggregate: k_confusion adds the population count of the lanes that share a key once (default on; eval.hip).
bool opt_confusion_wave_aggregate();

// probs_labels_tiles: class-vector images whose layout allows it are arg-maxed from LDS tiles (default on; 0: every image takes the
// generic one-lane-per-pixel path; probs_labels.hip).  Same results either way: a test hook.
bool opt_probs_labels_tiles();
// resize_vector: class-vector images whose layout allows it are resampled with 16-byte loads and stores (default on; 0: every image
// takes the generic one-lane-per-element path; resize.hip).  Same results either way: a test hook.
bool opt_resize_vector();
// lens_vector: class-vector images whose layout allows it are undistorted with 16-byte loads and stores and one map per pixel in LDS
// (default on; 0: every image takes the generic one-lane-per-element path; lens.hip).  Same results either way: a test hook.
bool opt_lens_vector();
// fuse_sampled: the entry points of smesh_sampled.h sample (w,h,C) class vectors inside k_fuse_tri_sampled where it serves the view
// (default on; 0 / SMESH_FUSE_SAMPLED=0: every call resamples, then fuses; fusion_sampled.hip).  Same sums either way: a test hook.
bool opt_fuse_sampled();
// points_grid: smesh_surface_index_nearest walks the index's grid (default on; 0: the exhaustive scan, one lane per point over all faces;
// points.hip).  Same results either way: a test hook and the baseline of tools/point_transfer_bench.py.
bool opt_points_grid();
// Largest class count the tiled path of probs_labels.hip serves.  Read-only option "probs_labels_tile_max_classes".
constexpr uint32_t kProbsLabelsTileMaxC = 255;

// Largest class count whose confusion matrix a workgroup of k_confusion keeps as a private uint32 histogram in LDS (eval.hip, where
// the budget is stated and this value is checked against it).  Read-only option "confusion_lds_max_classes" (smesh_get_option).
constexpr uint32_t kConfusionLdsMaxC = 180;

// Grow-only device scratch buffer.
struct Scratch {
  void* ptr = nullptr;
  size_t bytes = 0;
  int reserve(size_t need);
  void release();
};

inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// An integer setting from the environment (atoi), `def` when the variable is unset.
inline int env_int(const char* name, int def) {
  const char* e = getenv(name);
  return e ? atoi(e) : def;
}

// Per-triangle record the rasteriser leaves for the triangle-order fusion (smesh_fuse_view):
//   kind 1 (small): bounding box at (x0, y0) of at most 8 x 8 pixels; bit (dx * 8 + dy) of `mask` is set when
//                   the triangle emitted a fragment at (x0 + dx, y0 + dy) (it may still have lost the depth test);
//   kind 2 (big):   bounding box (x0, y0) .. (x1, y1) with x1 = mask & 0xFFFF, y1 = (mask >> 16) & 0xFFFF;
//   kind 0:         culled / nothing emitted.
struct TriFrag {
  uint16_t x0, y0;
  uint16_t kind;
  uint16_t pad;
  unsigned long long mask;
};
static_assert(sizeof(TriFrag) == 16, "TriFrag must be 16 bytes");

// Arguments of the triangle-order fusion kernels (fuse_tri.inc.hpp, fusion.hip).
struct TriFuseArgs {
  const TriFrag* frags;
  const uint32_t* idx;
  const float* probs;
  const float* weights;       // may be null
  float* acc;                 // [P][C] dense
  float* acc_lo;              // Mul only: second float32 plane, a row's value is acc + acc_lo (fuse_tri.inc.hpp, "Mul state"); else null
  uint64_t F;
  uint32_t C, W, H;
  float iew;
  const uint32_t* big_queue;
  const uint32_t* big_len;    // queue length of this render (emptied by the next render's vertex kernel)
  uint32_t big_capacity;
  uint32_t tri_blocks;        // blocks 0 .. tri_blocks-1 walk the triangles, the next big_blocks the big-triangle queue, the rest (k_fuse_tri with `mid`) the lists of medium triangles
  uint32_t big_blocks;
  uint32_t compact = 0u;      // k_fuse_tri only, launch-uniform: nonzero = every view's `frags` is the two-plane allocation of records.hpp (8-byte words,
                              // the TriFrag of kinds 2 and 3 behind them); 0 = [F] TriFrag
  const uint32_t* prim_id;    // [F] primitive id of triangle f when the renderer re-ordered its triangles (null: id == f)
  // texel primitives (k_fuse_texel) only
  const uint32_t* tex_first;  // [F] first texel id of each triangle
  const uint32_t* tex_res;    // [F] texel resolution r: the triangle owns r (r + 1) / 2 consecutive texels
  const uint8_t* tex_kinds;   // [F] TriFrag::kind of every triangle, a byte each: a texel renderer leaves a record only where it is nonzero
  uint32_t* count;            // [P] scratch histogram, all zero between launches (big triangles only)
  double* acc_d;              // Mul + texel primitives: [P][C] sums of ONE view's terms, all zero between launches (big triangles only)
  int mid;                    // k_fuse_tri: nonzero = the launch's last workgroups (fuse_mid_entries) take the queued triangles with at most kMidBox pixels per view (the tail waves skip them)
  uint32_t ps0, ps1;          // k_fuse_tri / fuse_box only: element strides of x and y of the class-vector image (dense: H * C and C); the class stride is 1
  // Fusion by triangle RANGE (smesh_fuse_views_begin / _continue: the rows of a finished range are exchanged between GPUs while the
  // next range is fused).  Main block b of the launch takes the triangles of block blk_first + b; the waves that walk the queues of
  // big triangles take only triangles at positions [f_lo, f_hi).  A launch over everything: blk_first = 0, f_lo = 0, f_hi = F.
  uint32_t blk_first;
  uint32_t f_lo, f_hi;
  uint32_t lds_pad;           // host side only: dynamic LDS of the eight-view k_fuse_tri launch (caps its workgroups per CU beside the rasteriser, fusion_multi8.hip)
};

// What k_fuse_tri needs to know about ONE of the views it fuses in a launch (the per-view part of TriFuseArgs), and NV of them.
struct TriView {
  const TriFrag* frags;
  const uint32_t* idx;
  const float* probs;
  const float* weights;       // may be null
  const uint32_t* big_queue;
  const uint32_t* big_len;    // [0] queue length, [1] "check the masks against the index plane" flag of the render
  uint32_t W, H;
  uint32_t ps0, ps1;          // k_fuse_tri only: element strides of x and y of `probs` (dense: H * C and C; a (H,W,C) tensor seen as (W,H,C): C and W * C)
  const uint8_t* kinds;       // k_fuse_texel_multi only: TriFrag::kind of every triangle, a byte each (null: read the records)
};
template <int NV>
struct TriViews {
  TriView v[NV];
};

// One rendered view as the triangle-order fusion consumes it (raster.hip -> fusion.hip).
struct RenderedView {
  const TriFrag* frags;         // per-triangle fragment records of the render
  const uint32_t* big_queue;    // triangles with a bounding box over 8 x 8 pixels ...
  const uint32_t* big_len;      // ... and how many (device counter)
  const uint32_t* idx;          // index plane [W][H]
  const float* probs;           // [W][H][C], device
  const float* weights;         // [W][H] or null, device
  uint64_t W, H;
  int64_t ps0 = 0, ps1 = 0;     // element strides of x and y of `probs` when it is not the dense (W,H,C) image (class stride 1); 0, 0: dense
  bool mid_queue = false;       // big_queue[big_capacity ...] lists the medium triangles of this view, big_len[3] of them (the rasteriser's renders)
  bool no_big = false;          // PROVEN on the host (raster.hip no_big_possible): no triangle of this view has a box over 8 x 8 pixels -- big_queue is empty
  const uint8_t* kinds = nullptr;   // texel renderers: TriFrag::kind of every triangle again, a byte each (RasterArgs::kinds)
  bool fine = false;            // bounded on the host (raster.hip box_extent_bound <= 48 pixels): a finely tessellated mesh seen from outside -- few or no queued triangles
  PipelineNeighbour beside;     // group pipeline: what the renderer's next group runs beside this view's fusion launch (raster.hip; zeros: unknown)
  const void* image = nullptr;  // what stands in for `probs` in the views of k_fuse_tri_labels, k_fuse_tri_h16 and k_fuse_tri_sampled: the dense label
                                // plane [W][H], the 16-bit image [W][H][C] (strides: ps0, ps1), the network's (w,h,C) image (view_input.hpp)
  bool compact = false;         // `frags` holds compact records (records.hpp): only smesh_aggregator_fuse_triangles' k_fuse_tri launches read them
};

// Medium triangles: a bounding box over 8 x 8 pixels of at most kMidBox pixels (16 x 16: beyond that a whole wave per triangle --
// fuse_box -- is faster than sixteen lanes, tools/mesh_density_sweep.py).  The rasteriser lists them (push_mid), the last workgroups of the k_fuse_tri launch fuse them (fuse_mid.inc.hpp).
constexpr int kMidBox = 256;

// Per-primitive records built from an arbitrary index image (image_records.hip): what lets MeshAggregator::add() run the
// triangle-order fusion on images the library did not render.  Scratch of one aggregator, all zero between calls.
struct ImageRecords {
  TriFrag* frags = nullptr;        // [P] (start of the one allocation)
  uint32_t* cand = nullptr;        // [P] ~(x << 16 | y) of the primitive's first pixel in (x, y) order; 0 = none
  uint4* big4 = nullptr;           // [P] primitives with runs outside the 8 x 8 box: largest x + 1, largest y + 1, pixels in those
                                   //     runs, 65536 - smallest y; zero otherwise
  uint32_t* big_queue = nullptr;   // [P] those primitives
  uint32_t* big_count = nullptr;   // [4] [0] queue length, [1] stays 0: the masks are exact, [2] nonzero: there are sparse primitives
  unsigned long long* mom = nullptr;   // [P] moments of the current image (count | sum x << 24 | sum y << 44), zero between calls
  uint64_t P = 0;
  bool clean = false;              // frags / cand / counters are all zero (what passes A and B start from)
  bool moments = false;            // the last build took passes M / R (image_records.hip)
  uint32_t tag = 2;                // passes M / R: what marks a record written by THIS call's pass M (alternates 2, 4)
  void release();
};
int image_records_build(DeviceCtx* ctx, ImageRecords& r, const uint32_t* d_idx, uint64_t W, uint64_t H, uint64_t P);
int image_records_pending(DeviceCtx* ctx, ImageRecords& r, const uint32_t* d_idx, uint64_t W, uint64_t H, hipStream_t st);
int image_records_scatter_sparse(DeviceCtx* ctx, ImageRecords& r, int kind, const uint32_t* d_idx, const float* d_probs, const float* d_w,
                                 uint64_t W, uint64_t H, uint32_t C, float iew, float* acc, float* acc_lo, double* acc_d, hipStream_t st);
int image_records_clear(DeviceCtx* ctx, ImageRecords& r, const uint32_t* d_idx, uint64_t W, uint64_t H, hipStream_t st);
bool image_records_build_group(DeviceCtx* ctx, ImageRecords* const* recs, const uint32_t* const* d_idx, int n, uint64_t W, uint64_t H, uint64_t P,
                               int* status);
int image_records_scatter_sparse_group(DeviceCtx* ctx, ImageRecords* const* recs, int n, int kind, const uint32_t* const* d_idx,
                                       const float* const* d_probs, const float* const* d_w, uint64_t W, uint64_t H, uint32_t C, float iew,
                                       float* acc, float* acc_lo, double* acc_d, hipStream_t st);

}  // namespace smesh

// What the per-vertex results (vertices.hip) need from the handles that fusion.hip and raster.hip define.
struct smesh_aggregator;
struct smesh_renderer;
// Runs `use(ctx, rows, P, C)` on what get() would return -- the normalised float32 [P][C] result in the aggregator's device scratch,
// queued on the context's main stream -- with the aggregator and its context locked.  Obeys get()'s rules: a pending row exchange is
// joined first, a reduce-scattered accumulator is refused.
int smesh_aggregator_with_final_rows(smesh_aggregator* a,
                                     const std::function<int(smesh::DeviceCtx* ctx, const float* rows, uint64_t P, uint32_t C)>& use);
// The device tables of a texel renderer's layout: [F] first texel and resolution of every face, P texels in all.  SMESH_ERR_INVALID
// for a renderer of triangle primitives.
int smesh_renderer_texel_tables(const smesh_renderer* r, smesh::DeviceCtx** ctx, uint64_t* F, uint64_t* P, const uint32_t** first,
                                const uint32_t** res);
// The label of every row of a dense float32 [n, C] device array by the rule of smesh_vertices.h for a vertex with that one row
// (vertices.hip: k_vertex_gather, one row per item); `out_labels`: int32[n] in `out_memkind`.  Context locked, device current.
int smesh_rows_labels(smesh::DeviceCtx* ctx, const float* d_rows, uint64_t n, uint32_t C, float dont_care_threshold, int32_t* out_labels,
                      int out_memkind);
// What the face graph (face_graph.hip) needs from vertices.hip.  smesh_rows_finish: every row of a dense float32 [n, C] device array
// treated as a vertex with that one row is (mode, threshold; rows and/or labels, in `out_memkind`) -- smesh_rows_labels with rows.
// smesh_vertex_map_tables: the device CSR of a vertex map (uint32 offsets[V + 1], list[nnz]).  Context locked, device current.
struct smesh_vertex_map;
int smesh_rows_finish(smesh::DeviceCtx* ctx, const float* d_rows, uint64_t n, uint32_t C, int mode, float dont_care_threshold,
                      float* out_rows, int32_t* out_labels, int out_memkind);
int smesh_vertex_map_tables(const smesh_vertex_map* m, smesh::DeviceCtx** ctx, const uint32_t** offsets, const uint32_t** list);
// What the segments (face_segments.hip) need from face_graph.hip: the device CSR of a face graph (uint32 offsets[F + 1],
// neighbours[nnz]) and the context it lives in.
struct smesh_face_graph;
int smesh_face_graph_tables(const smesh_face_graph* graph, smesh::DeviceCtx** ctx, const uint32_t** offsets, const uint32_t** neighbours,
                            uint64_t* F, uint64_t* nnz);
// What the per-segment results (segment_stats.hip) need from face_segments.hip: the device tables of a set of segments, and the slot
// of its member table.  The member table belongs to the handle, which frees it; segment_stats.hip builds it on first use with the
// context locked: offsets[S + 1] (the exclusive scan of size), members[labelled] (every segment's faces, ascending, back to back),
// chunk_start[S + 1] (the exclusive scan of ceil(size / 256)), partial_start[S + 1] (the same over the segments of more than one
// chunk), and the two totals.
namespace smesh {
struct SegmentMembers {
  uint32_t *offsets = nullptr, *members = nullptr, *chunk_start = nullptr, *partial_start = nullptr;
  uint64_t chunks = 0, partials = 0;
  bool built = false;
};
struct SegmentTables {
  DeviceCtx* ctx;
  uint64_t F, S, labelled;
  const int32_t* ids;       // [F]
  const int32_t* labels;    // [F]
  const uint32_t* size;     // [S]
  SegmentMembers* members;
};
}  // namespace smesh
struct smesh_face_segments;
int smesh_face_segments_tables(smesh_face_segments* segments, smesh::SegmentTables* out);
// What the confusion matrices (eval.hip) need from a renderer: `n` views (at most eight) rasterised on the context's main stream with
// FULLY WRITTEN index planes, and `use(view, idx, W, H)` called for each with the renderer and its context locked -- what `use`
// queues on the main stream reads the plane before anything overwrites it.  `P` must be the renderer's primitive count.
int smesh_renderer_with_index_planes(smesh_renderer* r, const smesh_camera_t* cams, int n, uint64_t P, smesh::DeviceCtx* ctx,
                                     const std::function<int(int view, const uint32_t* idx, uint64_t W, uint64_t H)>& use);
