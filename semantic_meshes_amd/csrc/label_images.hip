// label_images.hip -- the fused mesh rendered back into the views as label and colour images (include/smesh_label_images.h): the
// kernel that turns an index plane and a per-primitive table into images in either orientation, and the entry points that feed it
// from an index image that already exists and from views rasterised here.
//
// Reference: README step 4 and eval-scannet/eval_scannet.py:301-320 (every frame rendered again, tf.gather(annotations,
// primitive_indices) into a (H,W,C) float image, argmax, palette, PNG).  Here the snapshot of a label renderer is resolved ONCE into
// one word per primitive that holds the output label and the output colour, so a pixel is one gather and a few byte moves.
#include "common.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/smesh_label_images.h"

using namespace smesh;

struct smesh_label_renderer {
  DeviceCtx* ctx = nullptr;
  uint64_t P = 0;
  uint32_t K = 0;
  int label_bytes = 1;            // 1: SMESH_LBL_U8, entries are uint32; 2: SMESH_LBL_U16, entries are uint64
  bool has_palette = false;
  uint64_t dc_entry = 0;          // the entry of every pixel without a valid label
  void* d_table = nullptr;        // [max(P, 1)] entries
  Scratch stage_idx, stage_out;   // device copies of HOST index images, device images behind HOST outputs
  std::mutex mu;                  // held for a whole entry point; taken before the renderer's and the context's locks
};

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;                       // pixels per thread, their loads in flight together
constexpr int kRows = 32, kRowLen = 128;             // a tile: 32 OUTPUT rows of 128 pixels (HW: 128 x by 32 y; WH: 32 x by 128 y)
static_assert(kRows * kRowLen == kThreads * kPerThread, "a tile is sixteen pixels per thread");
constexpr int kMaxViews = 8;
constexpr int kNotGrouped = -1000;                   // internal status of render_group: the planes came one at a time

// An entry: the output label in the low `8 * label_bytes` bits, then red, green, blue.
template <int LB> struct Entry;
template <> struct Entry<1> { using type = uint32_t; };
template <> struct Entry<2> { using type = uint64_t; };

struct ImageArgs {
  const void* idx[kMaxViews];     // index image of view blockIdx.z
  uint8_t* labels[kMaxViews];     // null for every view or for none
  uint8_t* colors[kMaxViews];     // likewise
  const void* table;
  uint64_t P;
  uint64_t dc_entry;
  int64_t is0, is1;               // element strides of x and y of the index images
  uint32_t W, H;
  int idx_dtype;
};

// A primitive index, widened: the background (0xFFFFFFFF, or -1 of a signed image) is >= every P the host accepts.
__device__ __forceinline__ uint64_t load_index(const void* p, int dt, uint64_t off) {
  switch (dt) {
    case SMESH_IDX_U32: return static_cast<const uint32_t*>(p)[off];
    case SMESH_IDX_I32: return (uint64_t)(int64_t) static_cast<const int32_t*>(p)[off];
    case SMESH_IDX_U64: return static_cast<const uint64_t*>(p)[off];
    default:            return (uint64_t) static_cast<const int64_t*>(p)[off];
  }
}

// Pitch in bytes of a tile row of BPP-byte pixels in LDS: the row, and up to three bytes in front of it (below).  In dwords it is
// odd -- 33, 65, 97 -- so the lanes of a wave that write one byte each into 32 different rows hit 32 different banks.
template <int BPP> constexpr int row_pitch() { return kRowLen * BPP + 4; }
static_assert((row_pitch<1>() / 4) % 2 == 1 && (row_pitch<2>() / 4) % 2 == 1 && (row_pitch<3>() / 4) % 2 == 1, "LDS row pitch must be odd");

// First byte of the part of output row `row` that belongs to the tile.
template <int BPP>
__device__ __forceinline__ uintptr_t segment(const uint8_t* out, uint64_t row, uint64_t pitch, uint32_t col0) {
  return reinterpret_cast<uintptr_t>(out) + (row * pitch + col0) * BPP;
}

// The offset of that byte within a dword of the output: the low two bits of its address, in 32-bit arithmetic.
template <int BPP>
__device__ __forceinline__ uint32_t misalign(const uint8_t* out, uint32_t row, uint32_t pitch, uint32_t col0) {
  return ((uint32_t)reinterpret_cast<uintptr_t>(out) + (row * pitch + col0) * BPP) & 3u;
}

// The tile's rows leave LDS a dword per lane.  Row r was written into LDS at the byte offset its first byte has within a dword of
// the OUTPUT (`seg & 3`), so a dword of LDS is a dword of the output: a whole store where all four bytes belong to the row's
// segment, byte stores for the up to three bytes at its head and its tail.  Nothing outside [seg, seg + nbytes) is written.
template <int BPP>
__device__ __forceinline__ void write_rows(const uint32_t* lds, uint8_t* out, uint32_t nrows, uint32_t len, uint64_t row0,
                                           uint64_t pitch, uint32_t col0) {
  constexpr uint32_t S = row_pitch<BPP>() / 4;      // dwords per LDS row
  const uint32_t nbytes = len * BPP;
  for (uint32_t j = threadIdx.x; j < nrows * S; j += kThreads) {
    const uint32_t r = j / S, s = j - r * S;
    const uintptr_t seg = segment<BPP>(out, row0 + r, pitch, col0);
    const uint32_t m = (uint32_t)(seg & 3u);
    const uint32_t lo = 4u * s, end = m + nbytes;   // this dword holds bytes [lo, lo + 4) of [m, end)
    if (lo >= end) continue;
    const uint32_t word = lds[r * S + s];
    uint8_t* dst = reinterpret_cast<uint8_t*>(seg - m + lo);
    if (lo >= m && lo + 4u <= end) {
      *reinterpret_cast<uint32_t*>(dst) = word;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4; k++)
        if (lo + k >= m && lo + k < end) dst[k] = (uint8_t)(word >> (8u * k));
    }
  }
}

// The one image kernel.  LB: bytes of an output label.  HW: the outputs are (H,W) images -- a transpose of the plane --, else (W,H).
// GENERIC: index images of any SMESH_IDX_* dtype at any strides, else dense uint32 planes.  Workgroup (bx, by, v) takes one tile of
// view v: it reads the plane along y (coalesced: y is the fastest index of a plane), gathers the entries, puts their label and colour
// bytes into LDS where they lie in the output rows, and writes the rows out along their fastest index (write_rows).
template <int LB, bool HW, bool GENERIC>
__global__ __launch_bounds__(kThreads) void k_label_images(ImageArgs a) {
  using E = typename Entry<LB>::type;
  constexpr int TX = HW ? kRowLen : kRows, TY = HW ? kRows : kRowLen;
  __shared__ uint32_t lds_lab[kRows * row_pitch<LB>() / 4];
  __shared__ uint32_t lds_rgb[kRows * row_pitch<3>() / 4];
  const int v = blockIdx.z;
  const void* idx = a.idx[v];
  uint8_t* out_lab = a.labels[v];
  uint8_t* out_rgb = a.colors[v];
  const uint32_t x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const uint32_t tw = min((uint32_t)TX, a.W - x0), th = min((uint32_t)TY, a.H - y0);   // (the grid covers the image: both >= 1)
  const uint32_t row0 = HW ? y0 : x0, col0 = HW ? x0 : y0, nrows = HW ? th : tw, len = HW ? tw : th;
  const uint64_t pitch = HW ? a.W : a.H;
  const E* table = static_cast<const E*>(a.table);

  uint64_t pidx[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; j++) {
    const uint32_t p = (uint32_t)j * kThreads + threadIdx.x, xx = p / TY, yy = p % TY;
    pidx[j] = ~0ull;
    if (xx < tw && yy < th) {
      if (GENERIC) pidx[j] = load_index(idx, a.idx_dtype, (uint64_t)(x0 + xx) * (uint64_t)a.is0 + (uint64_t)(y0 + yy) * (uint64_t)a.is1);
      else pidx[j] = static_cast<const uint32_t*>(idx)[(uint64_t)(x0 + xx) * a.H + (y0 + yy)];
    }
  }
  E ent[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; j++) ent[j] = pidx[j] < a.P ? table[pidx[j]] : (E)a.dc_entry;
  uint8_t* lab8 = reinterpret_cast<uint8_t*>(lds_lab);
  uint8_t* rgb8 = reinterpret_cast<uint8_t*>(lds_rgb);
#pragma unroll
  for (int j = 0; j < kPerThread; j++) {
    const uint32_t p = (uint32_t)j * kThreads + threadIdx.x, xx = p / TY, yy = p % TY;
    if (xx < tw && yy < th) {
      const uint32_t r = HW ? yy : xx, c = HW ? xx : yy;
      if (out_lab) {
        const uint32_t m = misalign<LB>(out_lab, row0 + r, (uint32_t)pitch, col0);
        uint8_t* d = lab8 + r * row_pitch<LB>() + m + c * LB;
        d[0] = (uint8_t)ent[j];
        if (LB == 2) d[1] = (uint8_t)(ent[j] >> 8);
      }
      if (out_rgb) {
        const uint32_t m = misalign<3>(out_rgb, row0 + r, (uint32_t)pitch, col0);
        uint8_t* d = rgb8 + r * row_pitch<3>() + m + c * 3;
        d[0] = (uint8_t)(ent[j] >> (8 * LB));
        d[1] = (uint8_t)(ent[j] >> (8 * LB + 8));
        d[2] = (uint8_t)(ent[j] >> (8 * LB + 16));
      }
    }
  }
  __syncthreads();
  if (out_lab) write_rows<LB>(lds_lab, out_lab, nrows, len, row0, pitch, col0);
  if (out_rgb) write_rows<3>(lds_rgb, out_rgb, nrows, len, row0, pitch, col0);
}

// table[p] = the entry of labels[p]: that of its class where the label is one, else the don't-care entry.
template <typename E>
__global__ void k_resolve_labels(const int32_t* labels, uint64_t P, const E* class_entries, uint32_t K, E dc_entry, E* table) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int32_t l = labels[p];
  table[p] = (uint32_t)l < K ? class_entries[l] : dc_entry;      // (a negative label is a huge unsigned one: don't care)
}

size_t index_itemsize(int dt) { return dt <= SMESH_IDX_I32 ? 4 : 8; }
bool bad_mem(int m) { return m != SMESH_MEM_HOST && m != SMESH_MEM_DEVICE; }
bool bad_layout(int l) { return l != SMESH_LAYOUT_WH && l != SMESH_LAYOUT_HW; }
size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

int check_image_size(uint64_t W, uint64_t H) {
  if (W == 0 || H == 0 || W > 65536 || H > 65536 || W * H >= 0x7FFFFFFFull / 4) return fail(SMESH_ERR_INVALID, "image too large");
  return SMESH_OK;
}

bool is_dense(const int64_t* s, uint64_t W, uint64_t H) { return !s || ((s[0] == (int64_t)H || W == 1) && (s[1] == 1 || H == 1)); }

// What the outputs of a call must be: which of them, and whether the label renderer can give them.
int check_outputs(const smesh_label_renderer* lr, bool labels, bool colors, int layout, int out_mem) {
  if (bad_layout(layout)) return fail(SMESH_ERR_INVALID, "label images: unknown layout");
  if (bad_mem(out_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (!labels && !colors) return fail(SMESH_ERR_INVALID, "label images: no output");
  if (colors && !lr->has_palette) return fail(SMESH_ERR_INVALID, "label images: a colour image needs a palette");
  return SMESH_OK;
}

// Queues the images of `nv` views of one resolution on the context's main stream: one launch.  Context locked, device current.
int launch_images(smesh_label_renderer* lr, ImageArgs a, int nv, int layout, bool generic) {
  DeviceCtx* ctx = lr->ctx;
  a.table = lr->d_table;
  a.P = lr->P;
  a.dc_entry = lr->dc_entry;
  const bool hw = layout == SMESH_LAYOUT_HW;
  const dim3 g((uint32_t)div_up(a.W, hw ? kRowLen : kRows), (uint32_t)div_up(a.H, hw ? kRows : kRowLen), (uint32_t)nv), b(kThreads);
  ProfScope prof(ctx, SMESH_PROF_LABEL_IMAGES);
  prof_note(ctx, SMESH_PROF_LABEL_IMAGES, 1, (uint64_t)nv);
#define SMESH_LAUNCH_IMAGES(LB)                                                                                      \
  do {                                                                                                               \
    if (hw && generic) hipLaunchKernelGGL((k_label_images<LB, true, true>), g, b, 0, ctx->stream, a);               \
    else if (hw) hipLaunchKernelGGL((k_label_images<LB, true, false>), g, b, 0, ctx->stream, a);                    \
    else if (generic) hipLaunchKernelGGL((k_label_images<LB, false, true>), g, b, 0, ctx->stream, a);               \
    else hipLaunchKernelGGL((k_label_images<LB, false, false>), g, b, 0, ctx->stream, a);                           \
  } while (0)
  if (lr->label_bytes == 1) SMESH_LAUNCH_IMAGES(1);
  else SMESH_LAUNCH_IMAGES(2);
#undef SMESH_LAUNCH_IMAGES
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

// Where the kernel writes the outputs of `nv` views of W x H pixels: the caller's DEVICE arrays, or slices of `stage_out` behind
// HOST arrays (copy_staged brings those home).
struct Outputs {
  uint8_t* lab[kMaxViews] = {};
  uint8_t* rgb[kMaxViews] = {};
};

int place_outputs(smesh_label_renderer* lr, int nv, uint64_t W, uint64_t H, void* const* labels_out, uint8_t* const* colors_out, int out_mem,
                  Outputs* o) {
  if (out_mem == SMESH_MEM_DEVICE) {
    for (int v = 0; v < nv; v++) {
      o->lab[v] = labels_out ? static_cast<uint8_t*>(labels_out[v]) : nullptr;
      o->rgb[v] = colors_out ? colors_out[v] : nullptr;
    }
    return SMESH_OK;
  }
  const size_t nl = labels_out ? align_up(W * H * (size_t)lr->label_bytes) : 0, nc = colors_out ? align_up(W * H * 3) : 0;
  SMESH_TRY(lr->stage_out.reserve((nl + nc) * (size_t)nv));      // (growing frees the old block, which waits for the library's streams)
  uint8_t* base = static_cast<uint8_t*>(lr->stage_out.ptr);
  for (int v = 0; v < nv; v++) {
    o->lab[v] = labels_out ? base + (nl + nc) * (size_t)v : nullptr;
    o->rgb[v] = colors_out ? base + (nl + nc) * (size_t)v + nl : nullptr;
  }
  return SMESH_OK;
}

int copy_staged(smesh_label_renderer* lr, int nv, uint64_t W, uint64_t H, void* const* labels_out, uint8_t* const* colors_out, const Outputs& o) {
  hipStream_t st = lr->ctx->stream;
  for (int v = 0; v < nv; v++) {
    if (labels_out) SMESH_HIP(hipMemcpyAsync(labels_out[v], o.lab[v], W * H * (size_t)lr->label_bytes, hipMemcpyDeviceToHost, st));
    if (colors_out) SMESH_HIP(hipMemcpyAsync(colors_out[v], o.rgb[v], W * H * 3, hipMemcpyDeviceToHost, st));
  }
  SMESH_HIP(hipStreamSynchronize(st));      // host images are complete when the call returns
  return SMESH_OK;
}

ImageArgs plane_args(uint64_t W, uint64_t H) {
  ImageArgs a = {};
  a.W = (uint32_t)W;
  a.H = (uint32_t)H;
  a.is0 = (int64_t)H;
  a.is1 = 1;
  a.idx_dtype = SMESH_IDX_U32;
  return a;
}

// Views [first, first + m) of a call, m <= 8: rasterised together, their images written by one launch where the views share a
// resolution.  smesh_renderer_with_index_planes hands the planes over in one of two ways: all m of them after the views were
// rasterised together, each in a buffer of its own, or -- renderers whose views cannot share launches -- one at a time in ONE
// buffer that the next view overwrites.  Only the first way lets a launch wait for the last plane; a second plane at the address
// of the first gives the second way away before anything was launched, and the group is done again view by view (kNotGrouped).
// `*ungrouped` remembers that for the rest of ONE call: which way it is depends on the renderer, the resolution and the environment.
int render_group(smesh_label_renderer* lr, smesh_renderer* renderer, const smesh_camera_t* cams, int m, int layout,
                 void* const* labels_out, uint8_t* const* colors_out, int out_mem, bool* ungrouped) {
  DeviceCtx* ctx = lr->ctx;
  bool same = true;
  for (int v = 1; v < m; v++) same = same && cams[v].width == cams[0].width && cams[v].height == cams[0].height;
  if (m > 1 && same && !*ungrouped) {
    ImageArgs a = plane_args(cams[0].width, cams[0].height);
    Outputs o;
    const int s = smesh_renderer_with_index_planes(renderer, cams, m, lr->P, ctx, [&](int v, const uint32_t* d_idx, uint64_t W, uint64_t H) -> int {
      if (v > 0 && d_idx == a.idx[0]) return kNotGrouped;
      a.idx[v] = d_idx;
      if (v + 1 < m) return SMESH_OK;
      SMESH_TRY(place_outputs(lr, m, W, H, labels_out, colors_out, out_mem, &o));
      for (int u = 0; u < m; u++) { a.labels[u] = o.lab[u]; a.colors[u] = o.rgb[u]; }
      SMESH_TRY(launch_images(lr, a, m, layout, false));
      if (out_mem == SMESH_MEM_HOST) SMESH_TRY(copy_staged(lr, m, W, H, labels_out, colors_out, o));
      return SMESH_OK;
    });
    if (s != kNotGrouped) return s;
    *ungrouped = true;
  }
  // One rasteriser call per view unless the group is rasterised together: each plane is consumed before the next one is made.
  const int step = (m > 1 && !*ungrouped) ? m : 1;
  for (int i = 0; i < m; i += step) {
    SMESH_TRY(smesh_renderer_with_index_planes(renderer, &cams[i], step, lr->P, ctx, [&](int v, const uint32_t* d_idx, uint64_t W, uint64_t H) -> int {
      const int u = i + v;
      ImageArgs a = plane_args(W, H);
      Outputs o;
      void* const* lo = labels_out ? &labels_out[u] : nullptr;
      uint8_t* const* co = colors_out ? &colors_out[u] : nullptr;
      SMESH_TRY(place_outputs(lr, 1, W, H, lo, co, out_mem, &o));
      a.idx[0] = d_idx;
      a.labels[0] = o.lab[0];
      a.colors[0] = o.rgb[0];
      SMESH_TRY(launch_images(lr, a, 1, layout, false));
      if (out_mem == SMESH_MEM_HOST) SMESH_TRY(copy_staged(lr, 1, W, H, lo, co, o));
      return SMESH_OK;
    }));
  }
  return SMESH_OK;
}

template <typename E>
int resolve_table(smesh_label_renderer* lr, const int32_t* d_labels, const std::vector<uint64_t>& class_entries, void* d_classes) {
  DeviceCtx* ctx = lr->ctx;
  std::vector<E> h(class_entries.begin(), class_entries.end());
  SMESH_HIP(hipMemcpyAsync(d_classes, h.data(), h.size() * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
  SMESH_HIP(hipStreamSynchronize(ctx->stream));          // (`h` goes away)
  const uint32_t grid = (uint32_t)div_up(lr->P, 256);
  hipLaunchKernelGGL(k_resolve_labels<E>, dim3(grid), dim3(256), 0, ctx->stream, d_labels, lr->P, static_cast<const E*>(d_classes), lr->K,
                     (E)lr->dc_entry, static_cast<E*>(lr->d_table));
  SMESH_HIP(hipGetLastError());
  SMESH_HIP(hipStreamSynchronize(ctx->stream));          // the snapshot is taken: the caller's table and the scratch may go
  return SMESH_OK;
}

int build_table(smesh_label_renderer* lr, const int32_t* prim_labels, int labels_mem, const uint8_t* palette, const uint8_t* dc_color,
                uint32_t dc_label) {
  const int shift = 8 * lr->label_bytes;
  const auto entry = [&](uint32_t label, const uint8_t* rgb) {
    return (uint64_t)label | ((uint64_t)rgb[0] << shift) | ((uint64_t)rgb[1] << (shift + 8)) | ((uint64_t)rgb[2] << (shift + 16));
  };
  const uint8_t black[3] = {0, 0, 0};
  lr->dc_entry = entry(dc_label, dc_color ? dc_color : black);
  const size_t esize = lr->label_bytes == 1 ? 4 : 8;
  SMESH_HIP(dev_malloc(&lr->d_table, std::max<uint64_t>(lr->P, 1) * esize));
  if (lr->P == 0) return SMESH_OK;
  std::vector<uint64_t> classes(lr->K);
  for (uint32_t c = 0; c < lr->K; c++) classes[c] = entry(c, palette ? palette + 3 * (size_t)c : black);
  Scratch d_classes, d_labels;
  int s = d_classes.reserve(lr->K * esize);
  const int32_t* labels = prim_labels;
  if (s == SMESH_OK && labels_mem == SMESH_MEM_HOST) {
    s = d_labels.reserve(lr->P * 4);
    if (s == SMESH_OK) {
      const hipError_t e = hipMemcpyAsync(d_labels.ptr, prim_labels, lr->P * 4, hipMemcpyHostToDevice, lr->ctx->stream);
      if (e != hipSuccess) s = fail_hip(e, "hipMemcpyAsync", __FILE__, __LINE__);
      labels = static_cast<const int32_t*>(d_labels.ptr);
    }
  }
  if (s == SMESH_OK) s = lr->label_bytes == 1 ? resolve_table<uint32_t>(lr, labels, classes, d_classes.ptr) : resolve_table<uint64_t>(lr, labels, classes, d_classes.ptr);
  d_classes.release();
  d_labels.release();
  return s;
}

}  // namespace

extern "C" {

int smesh_label_renderer_create(const int32_t* prim_labels, uint64_t P, int labels_mem, uint32_t num_classes, int label_dtype,
                                uint32_t dont_care_label, const uint8_t* palette, const uint8_t dont_care_color[3], int device,
                                smesh_label_renderer_t** out) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (label_dtype != SMESH_LBL_U8 && label_dtype != SMESH_LBL_U16) return fail(SMESH_ERR_INVALID, "label images: the label dtype must be uint8 or uint16");
  const uint32_t top = label_dtype == SMESH_LBL_U8 ? 255u : 65535u;
  if (num_classes == 0) return fail(SMESH_ERR_INVALID, "label images: the class count must be positive");
  if (num_classes > top) return fail(SMESH_ERR_INVALID, "label images: " + std::to_string(num_classes) + " classes do not fit the label dtype");
  if (dont_care_label > top) return fail(SMESH_ERR_INVALID, "label images: the don't-care label does not fit the label dtype");
  if (P && !prim_labels) return fail(SMESH_ERR_INVALID, "NULL label table");
  if (P >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "label images: P must stay below 2^32 - 1");
  if (bad_mem(labels_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  smesh_label_renderer* lr = new smesh_label_renderer;
  lr->ctx = ctx;
  lr->P = P;
  lr->K = num_classes;
  lr->label_bytes = label_dtype == SMESH_LBL_U8 ? 1 : 2;
  lr->has_palette = palette != nullptr;
  const int s = build_table(lr, prim_labels, labels_mem, palette, dont_care_color, dont_care_label);
  if (s != SMESH_OK) {
    if (lr->d_table) (void)dev_free(lr->d_table);
    delete lr;
    return s;
  }
  *out = lr;
  return SMESH_OK;
}

int smesh_label_renderer_destroy(smesh_label_renderer_t* lr) {
  if (!lr) return SMESH_OK;
  {
    std::lock_guard<std::mutex> g(lr->mu);
    std::lock_guard<std::recursive_mutex> lock(lr->ctx->mu);
    int current = -1;
    (void)hipGetDevice(&current);
    (void)hipSetDevice(lr->ctx->device);
    lr->stage_idx.release();
    lr->stage_out.release();
    if (lr->d_table) (void)dev_free(lr->d_table);
    if (current >= 0 && current != lr->ctx->device) (void)hipSetDevice(current);   // (the caller's current device is what it was)
  }
  delete lr;
  return SMESH_OK;
}

int smesh_label_renderer_render_image(smesh_label_renderer_t* lr, const void* indices, int idx_dtype, const int64_t idx_strides[2],
                                      int idx_mem, uint64_t W, uint64_t H, int layout, void* labels_out, uint8_t* colors_out, int out_mem) {
  if (!lr) return fail(SMESH_ERR_INVALID, "NULL label renderer");
  SMESH_TRY(check_outputs(lr, labels_out != nullptr, colors_out != nullptr, layout, out_mem));
  if (W == 0 || H == 0) return SMESH_OK;
  if (!indices) return fail(SMESH_ERR_INVALID, "NULL index image");
  if (idx_dtype < 0 || idx_dtype > SMESH_IDX_I64) return fail(SMESH_ERR_INVALID, "bad index dtype");
  if (idx_strides && (idx_strides[0] < 0 || idx_strides[1] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  if (bad_mem(idx_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  SMESH_TRY(check_image_size(W, H));
  // (W, H <= 65536: with strides below 2^40 the span of an image is below 2^57 elements and its offsets cannot wrap)
  if (idx_strides && (idx_strides[0] >= (1ll << 40) || idx_strides[1] >= (1ll << 40))) return fail(SMESH_ERR_INVALID, "index image strides too large");
  std::lock_guard<std::mutex> g(lr->mu);
  DeviceCtx* ctx = lr->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const int64_t dense[2] = {(int64_t)H, 1};
  const int64_t* s = idx_strides ? idx_strides : dense;
  ImageArgs a = plane_args(W, H);
  a.idx[0] = indices;
  std::vector<uint8_t> gathered;          // a HOST image at wide strides, made dense here
  if (idx_mem == SMESH_MEM_HOST) {
    const size_t item = index_itemsize(idx_dtype);
    const uint64_t span = 1 + (W - 1) * (uint64_t)s[0] + (H - 1) * (uint64_t)s[1];
    const void* src = indices;
    size_t bytes = (size_t)span * item;
    if (span > 4 * W * H + 65536) {       // (a few columns of a wide array: gathering costs less than copying the span)
      gathered.resize((size_t)(W * H) * item);
      const uint8_t* in = static_cast<const uint8_t*>(indices);
      for (uint64_t x = 0; x < W; x++)
        for (uint64_t y = 0; y < H; y++)
          memcpy(&gathered[(size_t)(x * H + y) * item], in + (size_t)(x * (uint64_t)s[0] + y * (uint64_t)s[1]) * item, item);
      src = gathered.data();
      bytes = gathered.size();
      s = dense;
    }
    // otherwise the span the strides cover, copied as it is
    SMESH_TRY(lr->stage_idx.reserve(std::max<size_t>(bytes, 16)));
    SMESH_HIP(hipMemcpyAsync(lr->stage_idx.ptr, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (!gathered.empty()) SMESH_HIP(hipStreamSynchronize(ctx->stream));      // (`gathered` goes away)
    a.idx[0] = lr->stage_idx.ptr;
  }
  a.is0 = s[0];
  a.is1 = s[1];
  a.idx_dtype = idx_dtype;
  const bool generic = idx_dtype != SMESH_IDX_U32 || !is_dense(s == dense ? nullptr : s, W, H);
  Outputs o;
  void* const lo[1] = {labels_out};
  uint8_t* const co[1] = {colors_out};
  SMESH_TRY(place_outputs(lr, 1, W, H, labels_out ? lo : nullptr, colors_out ? co : nullptr, out_mem, &o));
  a.labels[0] = o.lab[0];
  a.colors[0] = o.rgb[0];
  SMESH_TRY(launch_images(lr, a, 1, layout, generic));
  if (out_mem == SMESH_MEM_HOST) SMESH_TRY(copy_staged(lr, 1, W, H, labels_out ? lo : nullptr, colors_out ? co : nullptr, o));
  else if (idx_mem == SMESH_MEM_HOST) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

int smesh_label_renderer_render_views(smesh_label_renderer_t* lr, smesh_renderer_t* renderer, const smesh_camera_t* cameras, uint64_t n,
                                      int layout, void* const* labels_out, uint8_t* const* colors_out, int out_mem) {
  if (!lr || !renderer || (n && !cameras)) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (bad_layout(layout)) return fail(SMESH_ERR_INVALID, "label images: unknown layout");
  if (bad_mem(out_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (n) SMESH_TRY(check_outputs(lr, labels_out != nullptr, colors_out != nullptr, layout, out_mem));
  for (uint64_t i = 0; i < n; i++) {
    if ((labels_out && !labels_out[i]) || (colors_out && !colors_out[i])) return fail(SMESH_ERR_INVALID, "label images: NULL output image");
    if (cameras[i].width == 0 || cameras[i].height == 0) return fail(SMESH_ERR_INVALID, "camera resolution must be in [1, 65536]");
    SMESH_TRY(check_image_size(cameras[i].width, cameras[i].height));
  }
  std::lock_guard<std::mutex> g(lr->mu);
  // (P, the device and every camera are checked against the renderer before anything is rasterised or written)
  SMESH_TRY(smesh_renderer_with_index_planes(renderer, cameras, 0, lr->P, lr->ctx, nullptr));
  bool ungrouped = false;
  for (uint64_t i = 0; i < n; i += kMaxViews) {
    const int m = (int)std::min<uint64_t>(kMaxViews, n - i);
    SMESH_TRY(render_group(lr, renderer, &cameras[i], m, layout, labels_out ? &labels_out[i] : nullptr, colors_out ? &colors_out[i] : nullptr, out_mem,
                           &ungrouped));
  }
  return SMESH_OK;
}

}  // extern "C"
