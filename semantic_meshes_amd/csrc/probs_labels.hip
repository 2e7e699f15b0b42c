// probs_labels.hip -- the labels of a class-vector image and their confusion matrix (include/smesh_probs_labels.h): the network's
// own per-pixel prediction, arg-maxed and counted against ground truth where the image is.
//
// Reference: eval-scannet/eval_scannet.py:113-117, :232-236 ("ImageNetwork": each frame's (H,W,C) prediction arg-maxed, a
// confusion-matrix metric against the frame's label image).  Here it is one streaming read of the image: W H C elements in, one
// label per pixel out and / or one histogram key per pixel into the workgroup's LDS histogram of confusion.hpp.
//
// The rule: best = r[0], label = 0; ascending c: r[c] > best replaces.  Optional don't-care test: the float32 sum in
// ascending class order from 0.0f, don't care iff sum < threshold.  Both are evaluated by ONE lane per pixel in class order, so no
// result depends on the path, the tile size or the launch shape.
#include "confusion.hpp"
#include "half_scratch.hpp"

#include <cmath>

#include "../../include/smesh_probs_labels.h"

using namespace smesh;

namespace {

constexpr int kPlBlock = 256;
// Tiled path: a workgroup stages the rows of `npix` consecutive pixels of a run -- npix C contiguous elements -- widened to float32
// in LDS, one row every `pitch` dwords.  pitch = C | 1 is odd, so the 32 lanes that a ds_read_b32 services together, each reading
// class c of its own row, fall on 32 different banks.  24 KiB of staging beside the 16 KiB histogram is 40 KiB: four workgroups
// (16 waves) per CU, each with the up to 24 KiB (float32) / 12 KiB (16-bit) of its NEXT tile in flight while it scans the current one
// (k_probs_labels_tiled).  Without the histogram: six workgroups.
constexpr uint32_t kStageWords = 6144;
// npix = min(kPlBlock, kStageWords / pitch): 256 pixels up to 23 classes, 149 at 40, 40 at 150, 24 at 255.  Beyond kProbsLabelsTileMaxC a tile
// would feed less than half a wave's lanes: the generic path takes those.
static_assert(kStageWords / (kProbsLabelsTileMaxC | 1u) >= 16, "a tile must hold at least sixteen rows");
// Runs shorter than npix / kMinRunShare pixels (with a gap between them) go to the generic path.
constexpr uint32_t kMinRunShare = 8;
constexpr int kGroupsPerCuCount = 4, kGroupsPerCuPlain = 6;
static_assert(kGroupsPerCuCount * (kStageWords + kLdsWordsSmall) * 4 <= 160 * 1024, "four counting workgroups must fit a CU's LDS");

// The calling thread's last launch, for reporting (the read-only options "last_probs_labels_grid" / "last_probs_labels_work").
thread_local uint64_t g_last_grid = 0, g_last_work = 0;

size_t probs_itemsize(int dt) { return dt == SMESH_PROBS_F32 ? 4 : 2; }

struct PlArgs {
  const void* probs;
  int64_t s0, s1, s2;           // element strides of x, y and the class
  const void* gt;               // counting only
  int64_t gs0, gs1;
  unsigned long long* counts;   // [C (C + 1) + 1]; counting only
  void* out;                    // label image of `out_dtype` (SMESH_LBL_U8 / _U16 / _I32), or null
  int64_t os0, os1;
  int32_t* lbl32;               // dense int32 (W,H), y fastest, -1 for don't care (the two-pass form's first pass), or null
  uint64_t run_stride;          // tiled: elements between the starts of two runs (not read when the image is one run)
  uint64_t L;                   // tiled: pixels of a contiguous run -- run_len, or W H when the runs follow each other without a gap
  uint64_t tiles_per_run, tiles;
  uint32_t W, H, C;
  uint32_t run_len;             // tiled: pixels along the run axis (H for y, W for x)
  uint32_t run_axis;            // tiled: 1: consecutive pixels of a run differ in y (the dense image), 0: in x (a (H,W,C) tensor)
  uint32_t npix, pitch;
  uint32_t dc_value;            // what `out` gets for a don't-care pixel (the low bits of the value for a narrower dtype)
  float thr;
  int use_sum;                  // 0: no don't-care test, no sum
  int dtype, gt_dtype, out_dtype;
  int aggregate;
};

typedef uint32_t pl_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float load_elem(const void* p, int dt, uint64_t off) {
  if (dt == SMESH_PROBS_F32) return static_cast<const float*>(p)[off];
  float lo, hi;
  unpack2((uint32_t) static_cast<const uint16_t*>(p)[off], dt == SMESH_PROBS_BF16, lo, hi);
  return lo;
}

// What one pixel leaves behind: its label in `out` / `lbl32`, its key in the histogram (g: its ground truth as load_class gives it).
// Every lane of the wave gets here together.
template <bool COUNT>
__device__ __forceinline__ void emit(const PlArgs& a, uint32_t* hist, bool on, uint32_t x, uint32_t y, uint32_t label, bool dc, uint32_t g) {
  const uint32_t C = a.C;
  if (on) {
    if (a.out) {
      const uint64_t o = (uint64_t)x * (uint64_t)a.os0 + (uint64_t)y * (uint64_t)a.os1;
      const uint32_t v = dc ? a.dc_value : label;
      if (a.out_dtype == SMESH_LBL_U8) static_cast<uint8_t*>(a.out)[o] = (uint8_t)v;
      else if (a.out_dtype == SMESH_LBL_U16) static_cast<uint16_t*>(a.out)[o] = (uint16_t)v;
      else static_cast<uint32_t*>(a.out)[o] = v;
    }
    if (a.lbl32) a.lbl32[(uint64_t)x * a.H + y] = dc ? -1 : (int32_t)label;
  }
  if (COUNT) {
    uint32_t key = C * (C + 1u);   // ignored
    if (on && g != kNoClass) key = g * (C + 1u) + (dc ? C : label);
    add_keys<true>(hist, a.counts, key, on, a.aggregate);
  }
}

template <bool COUNT>
__device__ __forceinline__ void hist_clear(uint32_t* hist, uint32_t nbins) {
  if (COUNT) {
    for (uint32_t b = threadIdx.x; b <= nbins; b += kPlBlock) hist[b] = 0u;
    __syncthreads();
  }
}
// Non-zero bins only, with 64-bit atomics into the global matrix: as k_confusion flushes.
template <bool COUNT>
__device__ __forceinline__ void hist_flush(const uint32_t* hist, unsigned long long* counts, uint32_t nbins) {
  if (COUNT) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b <= nbins; b += kPlBlock) {
      const uint32_t v = hist[b];
      if (v) atomicAdd(&counts[b], (unsigned long long)v);
    }
  }
}

// GENERIC path: any strides.  One lane per pixel, pixel i = (i / H, i % H), strided loads in class order.  Correct, not fast.
template <bool COUNT>
__global__ __launch_bounds__(kPlBlock) void k_probs_labels_generic(PlArgs a) {
  __shared__ uint32_t hist[COUNT ? kLdsWordsSmall : 1];
  const uint32_t C = a.C, nbins = C * (C + 1u);
  hist_clear<COUNT>(hist, nbins);
  const uint64_t n = (uint64_t)a.W * a.H;
  const uint64_t rounds = (n + kPlBlock - 1) / kPlBlock;
  for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
    const uint64_t i = r * kPlBlock + threadIdx.x;
    const bool on = i < n;
    uint32_t x = 0, y = 0, label = 0, g = kNoClass;
    bool dc = false;
    if (on) {
      x = (uint32_t)(i / a.H);
      y = (uint32_t)(i - (uint64_t)x * a.H);
      const uint64_t off = (uint64_t)x * (uint64_t)a.s0 + (uint64_t)y * (uint64_t)a.s1;
      float best = load_elem(a.probs, a.dtype, off);
      float t = 0.0f;
      if (a.use_sum) t += best;
      for (uint32_t c = 1; c < C; c++) {
        const float v = load_elem(a.probs, a.dtype, off + (uint64_t)c * (uint64_t)a.s2);
        if (a.use_sum) t += v;
        if (v > best) { best = v; label = c; }
      }
      dc = a.use_sum && t < a.thr;
      if (COUNT) g = load_class(a.gt, a.gt_dtype, (uint64_t)x * (uint64_t)a.gs0 + (uint64_t)y * (uint64_t)a.gs1, C);
    }
    emit<COUNT>(a, hist, on, x, y, label, dc, g);
  }
  hist_flush<COUNT>(hist, a.counts, nbins);
}


// One 16-byte piece of a tile -- elements e .. e + 16 / EB - 1 -- widened into the staging rows.  (pix, c): row and class of e.
template <int EB>
__device__ __forceinline__ void stage_vec(float* stage, const pl_u32x4 q, bool bf, uint32_t pix, uint32_t c, uint32_t C, uint32_t pitch) {
  constexpr int VE = 16 / EB;
  float v[VE];
  if constexpr (EB == 4) {
    v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
  } else {
    unpack2(q.x, bf, v[0], v[1]); unpack2(q.y, bf, v[2], v[3]); unpack2(q.z, bf, v[4], v[5]); unpack2(q.w, bf, v[6], v[7]);
  }
  uint32_t w = pix * pitch + c;
#pragma unroll
  for (int k = 0; k < VE; k++) {
    stage[w] = v[k];
    c++;
    w++;
    if (c == C) { c = 0; w += pitch - C; }
  }
}

// TILED path: class stride 1, one pixel axis with stride C.  Tile t of the launch: pixels first .. first + cnt - 1 of run t /
// tiles_per_run, whose rows are the cnt C contiguous elements at `p`.  Lane i of the workgroup loads the 16-byte pieces i, i + 256,
// ... of the 16-byte-aligned middle of that span; the elements before and after the middle -- fewer than two pieces -- go one per
// lane.  A base that is only element-aligned just has a longer head.
template <int EB>
struct Tile {
  const char* p;        // the tile's first element
  const char* safe;     // a 16-byte piece inside the tile's run: what a lane without a piece of its own loads (and drops)
  uint32_t run, first, cnt, n, head, nvec, tail;
};

template <int EB>
__device__ __forceinline__ Tile<EB> tile_of(const PlArgs& a, uint32_t tile) {
  constexpr uint32_t VE = 16 / EB;
  Tile<EB> T;
  const uint32_t tpr = (uint32_t)a.tiles_per_run;
  T.run = tile / tpr;
  T.first = (tile - T.run * tpr) * a.npix;
  const uint64_t left = a.L - T.first;
  T.cnt = left < (uint64_t)a.npix ? (uint32_t)left : a.npix;
  T.n = T.cnt * a.C;                                  // elements of the tile: at most kStageWords
  const char* run_base = static_cast<const char*>(a.probs) + (uint64_t)T.run * a.run_stride * (uint64_t)EB;
  T.safe = run_base + ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(run_base) & 15u)) & 15u);   // (a run is 32 bytes or more: the host sees to it)
  T.p = run_base + (uint64_t)T.first * a.C * (uint64_t)EB;
  T.head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(T.p) & 15u)) & 15u) / EB;
  if (T.head > T.n) T.head = T.n;
  T.nvec = (T.n - T.head) / VE;
  T.tail = T.head + T.nvec * VE;                      // elements [tail, n): after the middle
  return T;
}

// Issues every load of a tile: MAXV pieces and one single element per lane, ALL unconditional (a lane without work loads the run's
// safe piece / the tile's first element), so that the code between here and the first use is straight-line and the loads stay in
// flight across it.
template <int EB, int MAXV>
__device__ __forceinline__ void tile_load(const Tile<EB>& T, uint32_t t, pl_u32x4 (&q)[MAXV], uint32_t& hv) {
  const char* mid = T.p + (uint64_t)T.head * EB;
#pragma unroll
  for (int k = 0; k < MAXV; k++) {
    const uint32_t v = t + (uint32_t)k * kPlBlock;
    const char* src = v < T.nvec ? mid + (uint64_t)v * 16u : T.safe;
    q[k] = *reinterpret_cast<const pl_u32x4*>(src);
  }
  const uint32_t extra = T.head + (T.n - T.tail);
  const uint32_t e = t < extra ? (t < T.head ? t : T.tail + (t - T.head)) : 0u;
  if constexpr (EB == 4) hv = reinterpret_cast<const uint32_t*>(T.p)[e];
  else hv = (uint32_t) reinterpret_cast<const uint16_t*>(T.p)[e];
}

// The loaded tile into the staging rows, widened.
template <int EB, int MAXV>
__device__ __forceinline__ void tile_stage(const Tile<EB>& T, uint32_t t, const pl_u32x4 (&q)[MAXV], uint32_t hv, float* stage, bool bf,
                                           uint32_t C, uint32_t pitch, uint32_t dq, uint32_t dr) {
  constexpr uint32_t VE = 16 / EB;
  if (t < T.head + (T.n - T.tail)) {                  // head and tail, one element per lane
    const uint32_t e = t < T.head ? t : T.tail + (t - T.head);
    const uint32_t pix = e / C;
    float lo, hi;
    if constexpr (EB == 4) lo = __uint_as_float(hv);
    else unpack2(hv, bf, lo, hi);
    stage[pix * pitch + (e - pix * C)] = lo;
  }
  const uint32_t e = T.head + t * VE;
  uint32_t pix = e / C, c = e - pix * C;
#pragma unroll
  for (int k = 0; k < MAXV; k++) {
    if (t + (uint32_t)k * kPlBlock < T.nvec) stage_vec<EB>(stage, q[k], bf, pix, c, C, pitch);
    pix += dq;      // a lane's pieces are kPlBlock VE elements apart: that many rows and classes further on
    c += dr;
    if (c >= C) { c -= C; pix++; }
  }
}

// A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  While it scans tile i out of LDS, the loads of its tile i + 1
// are in flight (issued after the rows of tile i were staged, into the same registers).  EB: bytes per element.
// MODE 0: labels only; 1: count against uint8 ground truth, whose load is one instruction that stays in flight with the pieces; 2:
// count against any ground truth (the loads sit in the branches of a switch, and the wave waits for them there, with the next tile's
// pieces queued before them: tools/probs_labels_bench.py measures the same images against uint16 ground truth).
// The staging stores are ds_write_b32 of 4 or 8 consecutive dwords per lane: across lanes a stride of 4 / 8 dwords, a 4- / 8-way bank
// conflict.  That is the probable reason why 16-bit images take the time of float32 ones; it has not been measured.
template <int EB, int MODE>
__global__ __launch_bounds__(kPlBlock) void k_probs_labels_tiled(PlArgs a) {
  constexpr bool COUNT = MODE != 0;
  constexpr uint32_t VE = 16 / EB;
  constexpr int MAXV = (int)(kStageWords / VE / kPlBlock);   // pieces per lane of the largest tile
  static_assert(MAXV * VE * kPlBlock == kStageWords, "the staging buffer is a whole number of pieces per lane");
  __shared__ float stage[kStageWords];
  __shared__ uint32_t hist[COUNT ? kLdsWordsSmall : 1];
  const uint32_t C = a.C, nbins = C * (C + 1u), pitch = a.pitch;
  const bool bf = a.dtype == SMESH_PROBS_BF16;
  hist_clear<COUNT>(hist, nbins);
  const uint32_t t = threadIdx.x;
  const uint32_t dq = (kPlBlock * VE) / C, dr = (kPlBlock * VE) - dq * C;
  const uint32_t tiles = (uint32_t)a.tiles;           // < 2^29
  uint32_t tile = blockIdx.x;                          // (the grid has at most `tiles` workgroups)
  Tile<EB> cur = tile_of<EB>(a, tile);
  pl_u32x4 q[MAXV];
  uint32_t hv, x, y;
  uint64_t gbits = 0;
  // this lane's pixel of a tile (a lane without one: the tile's first), and the bits of its ground truth
  auto pixel_of = [&](const Tile<EB>& T, uint32_t& px, uint32_t& py, uint64_t& bits) {
    const uint32_t pixel = T.run * (uint32_t)a.L + T.first + (t < T.cnt ? t : 0u);          // < W H < 2^29
    const uint32_t u = pixel / a.run_len, w = pixel - u * a.run_len;
    px = a.run_axis ? u : w;
    py = a.run_axis ? w : u;
    const uint64_t off = (uint64_t)px * (uint64_t)a.gs0 + (uint64_t)py * (uint64_t)a.gs1;
    if (MODE == 1) bits = static_cast<const uint8_t*>(a.gt)[off];
    else if (MODE == 2) bits = load_gt_bits(a.gt, a.gt_dtype, off);
  };
  tile_load<EB, MAXV>(cur, t, q, hv);
  pixel_of(cur, x, y, gbits);
  for (;;) {
    tile_stage<EB, MAXV>(cur, t, q, hv, stage, bf, C, pitch, dq, dr);
    const bool on = t < cur.cnt;
    const uint32_t g = COUNT ? class_of_bits(gbits, a.gt_dtype, C) : kNoClass;
    const uint32_t next = tile + gridDim.x;
    const bool more = next < tiles;
    // (the last round has no next tile: its loads stay, so that the code is straight-line, but every lane loads one and the same
    //  piece, element and ground-truth pixel of its own tile again -- a cache line or two per wave -- and drops them)
    Tile<EB> nxt = tile_of<EB>(a, more ? next : tile);
    if (!more) { nxt.nvec = 0; nxt.n = 0; nxt.head = 0; nxt.tail = 0; nxt.cnt = 0; }
    uint32_t xn, yn;
    tile_load<EB, MAXV>(nxt, t, q, hv);
    pixel_of(nxt, xn, yn, gbits);
    __syncthreads();
    // one lane per pixel, ascending class order
    uint32_t label = 0;
    bool dc = false;
    if (on) {
      const float* r = stage + t * pitch;
      float best = r[0];
      if (a.use_sum) {
        float sum = 0.0f;
        sum += best;
        for (uint32_t c = 1; c < C; c++) {
          const float v = r[c];
          sum += v;
          if (v > best) { best = v; label = c; }
        }
        dc = sum < a.thr;
      } else {
        for (uint32_t c = 1; c < C; c++) {
          const float v = r[c];
          if (v > best) { best = v; label = c; }
        }
      }
    }
    emit<COUNT>(a, hist, on, x, y, label, dc, g);
    if (!more) break;
    __syncthreads();   // (the next tile overwrites the rows)
    cur = nxt;
    tile = next;
    x = xn;
    y = yn;
  }
  hist_flush<COUNT>(hist, a.counts, nbins);
}

// The checks both entry points share; fills the image part of `a` (strides, shape, threshold).
int check_probs(PlArgs& a, const void* probs, int dt, const int64_t* s, int mem, uint64_t W, uint64_t H, uint32_t C, float thr) {
  if (!probs) return fail(SMESH_ERR_INVALID, "probs labels: NULL class-vector image");
  if (dt != SMESH_PROBS_F32 && dt != SMESH_PROBS_F16 && dt != SMESH_PROBS_BF16) return fail(SMESH_ERR_INVALID, "probs labels: bad class-vector dtype");
  if (s && (s[0] < 0 || s[1] < 0 || s[2] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (bad_mem(mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (reinterpret_cast<uintptr_t>(probs) % probs_itemsize(dt)) return fail(SMESH_ERR_INVALID, "probs labels: the image is not aligned to its element size");
  if (C == 0) return fail(SMESH_ERR_INVALID, "probs labels: the class count must be positive");
  if (thr != thr) return fail(SMESH_ERR_INVALID, "probs labels: the don't-care threshold is NaN");
  SMESH_TRY(check_image_size(W, H));
  a.s0 = s ? s[0] : (int64_t)(H * C);
  a.s1 = s ? s[1] : (int64_t)C;
  a.s2 = s ? s[2] : 1;
  a.W = (uint32_t)W;
  a.H = (uint32_t)H;
  a.C = C;
  a.dtype = dt;
  a.thr = thr;
  a.use_sum = (std::isinf(thr) && thr < 0) ? 0 : 1;
  return SMESH_OK;
}

int check_out(PlArgs& a, int out_dtype, const int64_t* os, int64_t dcv, uint64_t H, uint32_t C) {
  if (out_dtype != SMESH_LBL_U8 && out_dtype != SMESH_LBL_U16 && out_dtype != SMESH_LBL_I32)
    return fail(SMESH_ERR_INVALID, "probs labels: the label image must be uint8, uint16 or int32");
  if (os && (os[0] < 0 || os[1] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  const int64_t lo = out_dtype == SMESH_LBL_I32 ? -2147483648ll : 0;
  const int64_t hi = out_dtype == SMESH_LBL_U8 ? 255 : out_dtype == SMESH_LBL_U16 ? 65535 : 2147483647ll;
  if ((int64_t)C - 1 > hi || (out_dtype != SMESH_LBL_I32 && (int64_t)C > hi))
    return fail(SMESH_ERR_INVALID, "probs labels: the label dtype is too narrow for the class count");
  if (dcv < lo || dcv > hi) return fail(SMESH_ERR_INVALID, "probs labels: the label dtype cannot hold the don't-care value");
  if (dcv >= 0 && dcv < (int64_t)C) return fail(SMESH_ERR_INVALID, "probs labels: the don't-care value is a class");
  a.out_dtype = out_dtype;
  a.os0 = os ? os[0] : (int64_t)H;
  a.os1 = os ? os[1] : 1;
  a.dc_value = (uint32_t)(int32_t)dcv;
  return SMESH_OK;
}

// Which path: fills the tile geometry when the tiled one serves the image.
bool plan_tiles(PlArgs& a) {
  if (!opt_probs_labels_tiles() || a.C > kProbsLabelsTileMaxC || (a.s2 != 1 && a.C != 1)) return false;
  const uint64_t C = a.C;
  uint64_t runs;
  const bool by_y = (uint64_t)a.s1 == C || (a.W == 1 && a.H == 1), by_x = (uint64_t)a.s0 == C;
  if (by_y && (!by_x || a.H >= a.W)) {                 // (both: the axis with the longer run)
    a.run_axis = 1; a.run_len = a.H; runs = a.W; a.run_stride = (uint64_t)a.s0;
  } else if (by_x) {
    a.run_axis = 0; a.run_len = a.W; runs = a.H; a.run_stride = (uint64_t)a.s1;
  } else {
    return false;
  }
  a.L = a.run_len;
  if (runs == 1 || a.run_stride == (uint64_t)a.run_len * C) {   // the runs follow each other without a gap: one run
    a.L = (uint64_t)a.W * a.H;
    runs = 1;
    a.run_stride = 0;
  }
  if (a.L * C * probs_itemsize(a.dtype) < 32) return false;      // (k_probs_labels_tiled needs a 16-byte piece inside every run)
  a.pitch = a.C | 1u;
  a.npix = std::min<uint32_t>(kPlBlock, kStageWords / a.pitch);
  if (runs > 1 && a.L * kMinRunShare < a.npix) return false;                // (runs that fill under an eighth of a tile: one lane per pixel serves them better)
  a.tiles_per_run = div_up(a.L, a.npix);
  a.tiles = runs * a.tiles_per_run;
  return true;
}

// Queues the kernel on the context's main stream, inside profile slot 7.  Context locked, device current, `a` checked; counting
// (a.counts set) needs C <= 63.
int launch_probs_labels(DeviceCtx* ctx, PlArgs a) {
  const bool count = a.counts != nullptr;
  a.aggregate = opt_confusion_wave_aggregate() ? 1 : 0;
  const bool tiled = plan_tiles(a);
  const uint64_t work = tiled ? a.tiles : div_up((uint64_t)a.W * a.H, kPlBlock);
  const uint64_t cap = (uint64_t)std::max(1, ctx->num_cus) * (uint64_t)(count ? kGroupsPerCuCount : kGroupsPerCuPlain);
  const dim3 g((uint32_t)std::min(work, cap)), b(kPlBlock);
  ProfScope prof(ctx, SMESH_PROF_PROBS_LABELS);
  prof_note(ctx, SMESH_PROF_PROBS_LABELS, 1, 1);
  if (tiled) {
    if (a.dtype == SMESH_PROBS_F32) {
      if (count && a.gt_dtype == SMESH_LBL_U8) hipLaunchKernelGGL((k_probs_labels_tiled<4, 1>), g, b, 0, ctx->stream, a);
      else if (count) hipLaunchKernelGGL((k_probs_labels_tiled<4, 2>), g, b, 0, ctx->stream, a);
      else hipLaunchKernelGGL((k_probs_labels_tiled<4, 0>), g, b, 0, ctx->stream, a);
    } else {
      if (count && a.gt_dtype == SMESH_LBL_U8) hipLaunchKernelGGL((k_probs_labels_tiled<2, 1>), g, b, 0, ctx->stream, a);
      else if (count) hipLaunchKernelGGL((k_probs_labels_tiled<2, 2>), g, b, 0, ctx->stream, a);
      else hipLaunchKernelGGL((k_probs_labels_tiled<2, 0>), g, b, 0, ctx->stream, a);
    }
  } else {
    if (count) hipLaunchKernelGGL(k_probs_labels_generic<true>, g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_probs_labels_generic<false>, g, b, 0, ctx->stream, a);
  }
  SMESH_HIP(hipGetLastError());
  g_last_grid = g.x; g_last_work = work;   // (reporting only)
  return SMESH_OK;
}

// A HOST class-vector image staged at its own width: the span its strides cover, as image_on_device stages a (W,H) image.
int probs_on_device(DeviceCtx* ctx, Scratch& stage, const PlArgs& a, const void* probs, int mem, const void** out, bool* staged) {
  *out = probs;
  if (mem == SMESH_MEM_DEVICE) return SMESH_OK;
  const uint64_t span = 1 + (uint64_t)(a.W - 1) * (uint64_t)a.s0 + (uint64_t)(a.H - 1) * (uint64_t)a.s1 + (uint64_t)(a.C - 1) * (uint64_t)a.s2;
  const size_t bytes = (size_t)span * probs_itemsize(a.dtype);
  SMESH_TRY(stage.reserve(std::max<size_t>(bytes, 16)));
  SMESH_HIP(hipMemcpyAsync(stage.ptr, probs, bytes, hipMemcpyHostToDevice, ctx->stream));
  *out = stage.ptr;
  *staged = true;
  return SMESH_OK;
}

struct ScratchGuard {     // scratch of one call of smesh_probs_labels
  Scratch s;
  ~ScratchGuard() { s.release(); }
};

}  // namespace

// (context.cpp: the read-only options "last_probs_labels_grid" / "last_probs_labels_work")
namespace smesh {
void smesh_last_probs_labels_launch(uint64_t* grid, uint64_t* work) { *grid = g_last_grid; *work = g_last_work; }
}  // namespace smesh

extern "C" {

int smesh_probs_labels(const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_mem, uint64_t W, uint64_t H, uint32_t C,
                       float dont_care_threshold, void* out, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value,
                       int out_mem, int device) {
  if (W == 0 || H == 0) return SMESH_OK;
  PlArgs a = {};
  SMESH_TRY(check_probs(a, probs, probs_dtype, probs_strides, probs_mem, W, H, C, dont_care_threshold));
  if (!out) return fail(SMESH_ERR_INVALID, "probs labels: NULL label image");
  if (bad_mem(out_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  SMESH_TRY(check_out(a, out_dtype, out_strides, dont_care_value, H, C));
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  ScratchGuard in, res;
  bool staged = false;
  SMESH_TRY(probs_on_device(ctx, in.s, a, probs, probs_mem, &a.probs, &staged));
  const size_t osize = label_itemsize(out_dtype);
  const int64_t os0 = a.os0, os1 = a.os1;
  if (out_mem == SMESH_MEM_HOST) {       // a dense device image, copied back below
    SMESH_TRY(res.s.reserve(std::max<size_t>((size_t)(W * H) * osize, 16)));
    a.out = res.s.ptr;
    a.os0 = (int64_t)H;
    a.os1 = 1;
  } else {
    a.out = out;
  }
  SMESH_TRY(launch_probs_labels(ctx, a));
  if (out_mem == SMESH_MEM_HOST) {
    if (is_dense(out_strides, W, H)) {
      SMESH_HIP(hipMemcpyAsync(out, res.s.ptr, (size_t)(W * H) * osize, hipMemcpyDeviceToHost, ctx->stream));
      SMESH_HIP(hipStreamSynchronize(ctx->stream));
    } else {
      std::vector<char> h((size_t)(W * H) * osize);
      SMESH_HIP(hipMemcpyAsync(h.data(), res.s.ptr, h.size(), hipMemcpyDeviceToHost, ctx->stream));
      SMESH_HIP(hipStreamSynchronize(ctx->stream));
      char* o = static_cast<char*>(out);
      for (uint64_t x = 0; x < W; x++)
        for (uint64_t y = 0; y < H; y++)
          std::copy_n(h.data() + (x * H + y) * osize, osize, o + (x * (uint64_t)os0 + y * (uint64_t)os1) * osize);
    }
  } else if (staged) {
    SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  }
  return SMESH_OK;
}

int smesh_confusion_add_probs(smesh_confusion_t* cm, const void* probs, int probs_dtype, const int64_t probs_strides[3], int probs_mem,
                              const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_mem, uint64_t W, uint64_t H,
                              float dont_care_threshold, void* labels_out, int out_dtype, const int64_t out_strides[2], int64_t dont_care_value) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  if (W == 0 || H == 0) return SMESH_OK;
  PlArgs a = {};
  SMESH_TRY(check_probs(a, probs, probs_dtype, probs_strides, probs_mem, W, H, cm->C, dont_care_threshold));
  SMESH_TRY(check_gt(gt, gt_dtype, gt_strides, gt_mem));
  if (labels_out) SMESH_TRY(check_out(a, out_dtype, out_strides, dont_care_value, H, cm->C));
  a.out = labels_out;
  std::lock_guard<std::mutex> g(cm->mu);
  DeviceCtx* ctx = cm->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  bool staged = false;
  SMESH_TRY(probs_on_device(ctx, cm->stage_src, a, probs, probs_mem, &a.probs, &staged));
  const void* d_gt = nullptr;
  SMESH_TRY(image_on_device(ctx, cm->stage_gt, gt, label_itemsize(gt_dtype), gt_strides, gt_mem, W, H, &d_gt, &staged));
  if (cm->nbins + 1 <= kLdsWordsSmall) {   // one pass: label and count (up to 63 classes)
    a.gt = d_gt;
    a.gt_dtype = gt_dtype;
    a.gs0 = gt_strides ? gt_strides[0] : (int64_t)H;
    a.gs1 = gt_strides ? gt_strides[1] : 1;
    a.counts = cm->d_counts;
    SMESH_TRY(launch_probs_labels(ctx, a));
  } else {                                 // two passes: int32 labels into scratch, then k_confusion in its labels mode
    SMESH_TRY(cm->stage_lbl.reserve((size_t)(W * H) * 4));
    a.lbl32 = static_cast<int32_t*>(cm->stage_lbl.ptr);
    SMESH_TRY(launch_probs_labels(ctx, a));
    SMESH_TRY(smesh_confusion_count_label_image(cm, a.lbl32, d_gt, gt_dtype, gt_strides, W, H));
  }
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

}  // extern "C"
