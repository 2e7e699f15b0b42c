// eval.hip -- confusion matrices of the fused mesh against ground truth (include/smesh_eval.h): the counting kernel, the primitive
// labels of an aggregator, and the entry points that feed the kernel from 1-D label arrays, from an index image that already exists
// and from views rasterised here.
//
// Reference: eval-scannet/eval_scannet.py:108-112, :286-287 (per vertex) and :301-316 (per pixel: every frame rendered again,
// tf.gather(annotations, primitive_indices) into a (H,W,C) float image, a confusion-matrix metric against the frame's label image).
// Here a sample is two small integers: the ground-truth class g and the predicted class p = prim_labels[index], and the matrix cell
// g (C + 1) + p gets one more.  Integer counts only: no result depends on launch shape, atomic order or batching.
#include "confusion.hpp"

using namespace smesh;

namespace {

constexpr int kBlock = 1024;      // 16 waves: a histogram over 80 KiB leaves room for ONE workgroup per CU, and it should fill the CU
constexpr int kPerThread = 4;     // samples per thread and step, their loads in flight together
constexpr uint32_t kTile = kBlock * kPerThread;
// A workgroup's uint32 bins cannot wrap: it takes at most kMaxTilesPerGroup tiles of kTile samples = 2^31 samples, and one bin gets
// at most all of them.  (The host raises the grid for inputs beyond num_cus * 2^31 samples.)
constexpr uint64_t kMaxTilesPerGroup = (1ull << 31) / kTile;
struct ConfArgs {
  const void* src;              // labels mode: int32 pred[n]; image mode: the index image
  const int32_t* prim_labels;   // image mode: int32[P]; null: labels mode
  uint64_t P;
  const void* gt;
  unsigned long long* counts;   // [C (C + 1) + 1]
  uint64_t n;                   // samples; image mode: W * H, sample i is pixel (i / H, i % H)
  int64_t is0, is1, gs0, gs1;   // element strides of x and y of the index image and of the ground truth
  uint32_t H;
  uint32_t C;
  int idx_dtype, gt_dtype;
  int idx_dense, gt_dense;      // the element of sample i is element i
  int aggregate;
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

// The one counting kernel: 1-D labels, an index image with a label gather, dense or strided ground truth of any label dtype.
// LDS_WORDS > 0: the workgroup's private uint32 histogram (C (C + 1) bins and `ignored`) lives in LDS, gets LDS integer atomics and
// is flushed at the end, non-zero bins only, with 64-bit atomics into the global matrix.  LDS_WORDS == 0: straight into the matrix.
// Workgroup b takes the tiles b, b + gridDim.x, ...: at most kMaxTilesPerGroup of them (the host sees to it).
template <uint32_t LDS_WORDS>
__global__ __launch_bounds__(kBlock) void k_confusion(ConfArgs a) {
  constexpr bool IN_LDS = LDS_WORDS > 0;
  __shared__ uint32_t hist[IN_LDS ? LDS_WORDS : 1];
  const uint32_t C = a.C;
  const uint32_t nbins = C * (C + 1u);          // bin `nbins`: ignored
  if (IN_LDS) {
    for (uint32_t b = threadIdx.x; b <= nbins; b += kBlock) hist[b] = 0u;
    __syncthreads();
  }
  const uint64_t tiles = (a.n + kTile - 1) / kTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t key[kPerThread];
    bool on[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; j++) {
      const uint64_t i = tile * kTile + (uint64_t)j * kBlock + threadIdx.x;
      on[j] = i < a.n;
      key[j] = nbins;
      if (on[j]) {
        uint64_t goff = i, ioff = i;
        if (!a.gt_dense || !a.idx_dense) {       // (images only: n < 2^29)
          const uint32_t x = (uint32_t)i / a.H, y = (uint32_t)i - x * a.H;
          if (!a.gt_dense) goff = (uint64_t)x * (uint64_t)a.gs0 + (uint64_t)y * (uint64_t)a.gs1;
          if (!a.idx_dense) ioff = (uint64_t)x * (uint64_t)a.is0 + (uint64_t)y * (uint64_t)a.is1;
        }
        const uint32_t g = load_class(a.gt, a.gt_dtype, goff, C);
        int32_t label;
        if (a.prim_labels) {
          const uint64_t idx = load_index(a.src, a.idx_dtype, ioff);
          label = idx < a.P ? a.prim_labels[idx] : -1;
        } else {
          label = static_cast<const int32_t*>(a.src)[ioff];
        }
        const uint32_t p = (uint32_t)label < C ? (uint32_t)label : C;   // (a negative label is a huge unsigned one: don't care)
        if (g != kNoClass) key[j] = g * (C + 1u) + p;
      }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; j++) add_keys<IN_LDS>(hist, a.counts, key[j], on[j], a.aggregate);
  }
  if (IN_LDS) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b <= nbins; b += kBlock) {
      const uint32_t v = hist[b];
      if (v) atomicAdd(&a.counts[b], (unsigned long long)v);
    }
  }
}

// Queues the count of a's samples on the context's main stream.  Context locked, device current, arguments checked.
int launch_confusion(smesh_confusion* cm, ConfArgs a) {
  if (a.n == 0) return SMESH_OK;
  DeviceCtx* ctx = cm->ctx;
  a.C = cm->C;
  a.counts = cm->d_counts;
  a.aggregate = opt_confusion_wave_aggregate() ? 1 : 0;
  const uint64_t tiles = div_up(a.n, kTile);
  const uint64_t grid = std::max<uint64_t>(std::min<uint64_t>(tiles, (uint64_t)std::max(1, ctx->num_cus)), div_up(tiles, kMaxTilesPerGroup));
  if (grid >= 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "confusion matrix: too many samples for one call");
  ProfScope prof(ctx, SMESH_PROF_CONFUSION);
  prof_note(ctx, SMESH_PROF_CONFUSION, 1, 1);
  const dim3 g((uint32_t)grid), b(kBlock);
  const uint64_t words = cm->nbins + 1;
  if (words <= kLdsWordsSmall) hipLaunchKernelGGL(k_confusion<kLdsWordsSmall>, g, b, 0, ctx->stream, a);
  else if (cm->C <= kConfusionLdsMaxC) hipLaunchKernelGGL(k_confusion<kLdsWordsLarge>, g, b, 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_confusion<0>, g, b, 0, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  return SMESH_OK;
}

size_t index_itemsize(int dt) { return dt <= SMESH_IDX_I32 ? 4 : 8; }

void set_gt(ConfArgs& a, const void* d_gt, int dt, const int64_t* strides, uint64_t W, uint64_t H) {
  a.gt = d_gt;
  a.gt_dtype = dt;
  a.gt_dense = is_dense(strides, W, H) ? 1 : 0;
  a.gs0 = strides ? strides[0] : (int64_t)H;
  a.gs1 = strides ? strides[1] : 1;
}

// One rendered view (a dense uint32 plane on the device) against its ground truth.  Context locked, device current.
int count_plane(smesh_confusion* cm, const uint32_t* d_idx, const int32_t* d_labels, uint64_t P, const void* gt, int gt_dtype,
                const int64_t* gt_strides, int gt_mem, uint64_t W, uint64_t H, bool* staged) {
  const void* d_gt = nullptr;
  SMESH_TRY(image_on_device(cm->ctx, cm->stage_gt, gt, label_itemsize(gt_dtype), gt_strides, gt_mem, W, H, &d_gt, staged));
  ConfArgs a = {};
  a.src = d_idx;
  a.prim_labels = d_labels;
  a.P = P;
  a.n = W * H;
  a.H = (uint32_t)H;
  a.idx_dtype = SMESH_IDX_U32;
  a.idx_dense = 1;
  a.is0 = (int64_t)H;
  a.is1 = 1;
  set_gt(a, d_gt, gt_dtype, gt_strides, W, H);
  return launch_confusion(cm, a);
}

}  // namespace

int smesh_confusion_count_label_image(smesh_confusion* cm, const int32_t* d_labels, const void* d_gt, int gt_dtype, const int64_t* gt_strides,
                                      uint64_t W, uint64_t H) {
  ConfArgs a = {};
  a.src = d_labels;
  a.n = W * H;
  a.H = (uint32_t)H;
  a.idx_dense = 1;
  a.is0 = (int64_t)H;
  a.is1 = 1;
  set_gt(a, d_gt, gt_dtype, gt_strides, W, H);
  return launch_confusion(cm, a);
}

extern "C" {

int smesh_confusion_create(uint32_t C, int device, smesh_confusion_t** out) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (C == 0) return fail(SMESH_ERR_INVALID, "confusion matrix: the class count must be positive");
  if ((uint64_t)C * (C + 1ull) >= 0x7FFFFFFFull) return fail(SMESH_ERR_INVALID, "confusion matrix: C (C + 1) must stay below 2^31");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  smesh_confusion* cm = new smesh_confusion;
  cm->ctx = ctx;
  cm->C = C;
  cm->nbins = (uint64_t)C * (C + 1ull);
  const hipError_t e = dev_malloc(reinterpret_cast<void**>(&cm->d_counts), (cm->nbins + 1) * 8);
  if (e != hipSuccess) { delete cm; return fail_hip(e, "hipMalloc confusion matrix", __FILE__, __LINE__); }
  const hipError_t e2 = hipMemsetAsync(cm->d_counts, 0, (cm->nbins + 1) * 8, ctx->stream);
  if (e2 != hipSuccess) { (void)dev_free(cm->d_counts); delete cm; return fail_hip(e2, "hipMemsetAsync", __FILE__, __LINE__); }
  *out = cm;
  return SMESH_OK;
}

int smesh_confusion_destroy(smesh_confusion_t* cm) {
  if (!cm) return SMESH_OK;
  {
    std::lock_guard<std::mutex> g(cm->mu);
    std::lock_guard<std::recursive_mutex> lock(cm->ctx->mu);
    int current = -1;
    (void)hipGetDevice(&current);
    (void)hipSetDevice(cm->ctx->device);
    cm->stage_src.release();
    cm->stage_gt.release();
    cm->stage_lbl.release();
    if (cm->d_counts) (void)dev_free(cm->d_counts);
    if (current >= 0 && current != cm->ctx->device) (void)hipSetDevice(current);   // (the caller's current device is what it was)
  }
  delete cm;
  return SMESH_OK;
}

int smesh_confusion_reset(smesh_confusion_t* cm) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  std::lock_guard<std::mutex> g(cm->mu);
  std::lock_guard<std::recursive_mutex> lock(cm->ctx->mu);
  SMESH_HIP(hipSetDevice(cm->ctx->device));
  SMESH_HIP(hipMemsetAsync(cm->d_counts, 0, (cm->nbins + 1) * 8, cm->ctx->stream));
  cm->merged.clear();
  return SMESH_OK;
}

int smesh_confusion_get(smesh_confusion_t* cm, uint64_t* counts, uint64_t* ignored) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  std::lock_guard<std::mutex> g(cm->mu);
  std::vector<uint64_t> h(cm->nbins + 1);
  {
    std::lock_guard<std::recursive_mutex> lock(cm->ctx->mu);
    SMESH_HIP(hipSetDevice(cm->ctx->device));
    SMESH_HIP(hipMemcpyAsync(h.data(), cm->d_counts, (cm->nbins + 1) * 8, hipMemcpyDeviceToHost, cm->ctx->stream));
    SMESH_HIP(hipStreamSynchronize(cm->ctx->stream));
  }
  if (!cm->merged.empty())
    for (uint64_t b = 0; b <= cm->nbins; b++) h[b] += cm->merged[b];
  if (counts) std::copy(h.begin(), h.begin() + cm->nbins, counts);
  if (ignored) *ignored = h[cm->nbins];
  return SMESH_OK;
}

int smesh_confusion_add_counts(smesh_confusion_t* cm, const uint64_t* counts, uint64_t ignored) {
  if (!cm || !counts) return fail(SMESH_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(cm->mu);
  if (cm->merged.empty()) cm->merged.assign(cm->nbins + 1, 0);
  for (uint64_t b = 0; b < cm->nbins; b++) cm->merged[b] += counts[b];
  cm->merged[cm->nbins] += ignored;
  return SMESH_OK;
}

int smesh_confusion_add_labels(smesh_confusion_t* cm, const int32_t* pred, int pred_mem, const void* gt, int gt_dtype, int gt_mem, uint64_t n) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  if (n == 0) return SMESH_OK;
  if (!pred) return fail(SMESH_ERR_INVALID, "NULL predictions");
  SMESH_TRY(check_gt(gt, gt_dtype, nullptr, gt_mem));
  if (bad_mem(pred_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (n >= (1ull << 48)) return fail(SMESH_ERR_INVALID, "confusion matrix: too many samples for one call");
  std::lock_guard<std::mutex> g(cm->mu);
  DeviceCtx* ctx = cm->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  bool staged = false;
  ConfArgs a = {};
  // (1-D arrays as images of one column: W = 1, so that the spans are n elements and everything is dense)
  SMESH_TRY(image_on_device(ctx, cm->stage_src, pred, 4, nullptr, pred_mem, 1, n, &a.src, &staged));
  const void* d_gt = nullptr;
  SMESH_TRY(image_on_device(ctx, cm->stage_gt, gt, label_itemsize(gt_dtype), nullptr, gt_mem, 1, n, &d_gt, &staged));
  a.n = n;
  a.H = 1;
  a.idx_dense = 1;
  set_gt(a, d_gt, gt_dtype, nullptr, 1, n);
  SMESH_TRY(launch_confusion(cm, a));
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

int smesh_aggregator_labels(smesh_aggregator_t* aggregator, float dont_care_threshold, int32_t* out, int memkind) {
  if (!aggregator) return fail(SMESH_ERR_INVALID, "NULL aggregator");
  if (bad_mem(memkind)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  return smesh_aggregator_with_final_rows(aggregator, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    if (P == 0) return SMESH_OK;
    if (!out) return fail(SMESH_ERR_INVALID, "labels: NULL output");
    return smesh_rows_labels(ctx, d_rows, P, C, dont_care_threshold, out, memkind);
  });
}

int smesh_confusion_add_image(smesh_confusion_t* cm, const void* indices, int idx_dtype, const int64_t idx_strides[2], int idx_mem,
                              const int32_t* prim_labels, uint64_t P, int labels_mem, const void* gt, int gt_dtype,
                              const int64_t gt_strides[2], int gt_mem, uint64_t W, uint64_t H) {
  if (!cm) return fail(SMESH_ERR_INVALID, "NULL confusion matrix");
  if (W == 0 || H == 0) return SMESH_OK;
  if (!indices) return fail(SMESH_ERR_INVALID, "NULL index image");
  if (idx_dtype < 0 || idx_dtype > SMESH_IDX_I64) return fail(SMESH_ERR_INVALID, "bad index dtype");
  if (idx_strides && (idx_strides[0] < 0 || idx_strides[1] < 0)) return fail(SMESH_ERR_INVALID, "negative strides are not supported");
  SMESH_TRY(check_gt(gt, gt_dtype, gt_strides, gt_mem));
  if (bad_mem(idx_mem) || bad_mem(labels_mem)) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (P && !prim_labels) return fail(SMESH_ERR_INVALID, "NULL label table");
  if (P >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "confusion matrix: P must stay below 2^32 - 1");
  SMESH_TRY(check_image_size(W, H));
  std::lock_guard<std::mutex> g(cm->mu);
  DeviceCtx* ctx = cm->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  bool staged = false;
  ConfArgs a = {};
  SMESH_TRY(image_on_device(ctx, cm->stage_src, indices, index_itemsize(idx_dtype), idx_strides, idx_mem, W, H, &a.src, &staged));
  const void* d_gt = nullptr;
  SMESH_TRY(image_on_device(ctx, cm->stage_gt, gt, label_itemsize(gt_dtype), gt_strides, gt_mem, W, H, &d_gt, &staged));
  const void* d_labels = prim_labels;
  if (P) SMESH_TRY(image_on_device(ctx, cm->stage_lbl, prim_labels, 4, nullptr, labels_mem, 1, P, &d_labels, &staged));
  // (an empty table: every pixel is don't care -- the kernel still tells the two modes apart by the pointer)
  a.prim_labels = P ? static_cast<const int32_t*>(d_labels) : reinterpret_cast<const int32_t*>(cm->d_counts);
  a.P = P;
  a.n = W * H;
  a.H = (uint32_t)H;
  a.idx_dtype = idx_dtype;
  a.idx_dense = is_dense(idx_strides, W, H) ? 1 : 0;
  a.is0 = idx_strides ? idx_strides[0] : (int64_t)H;
  a.is1 = idx_strides ? idx_strides[1] : 1;
  set_gt(a, d_gt, gt_dtype, gt_strides, W, H);
  SMESH_TRY(launch_confusion(cm, a));
  if (staged) SMESH_HIP(hipStreamSynchronize(ctx->stream));   // host arrays are consumed before the call returns
  return SMESH_OK;
}

int smesh_confusion_add_views(smesh_confusion_t* cm, smesh_renderer_t* renderer, const smesh_camera_t* cameras, uint64_t n,
                              const int32_t* prim_labels_dev, uint64_t P, const void* const* gts, int gt_dtype,
                              const int64_t gt_strides[2], int gt_mem) {
  if (!cm || !renderer || (n && (!cameras || !gts))) return fail(SMESH_ERR_INVALID, "NULL argument");
  if (P && !prim_labels_dev) return fail(SMESH_ERR_INVALID, "NULL label table");
  if (P >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "confusion matrix: P must stay below 2^32 - 1");
  for (uint64_t i = 0; i < n; i++) {
    SMESH_TRY(check_gt(gts[i], gt_dtype, gt_strides, gt_mem));
    if (cameras[i].width == 0 || cameras[i].height == 0) return fail(SMESH_ERR_INVALID, "camera resolution must be in [1, 65536]");
    SMESH_TRY(check_image_size(cameras[i].width, cameras[i].height));
  }
  std::lock_guard<std::mutex> g(cm->mu);
  // (P and the device are checked against the renderer before anything is rasterised or counted)
  SMESH_TRY(smesh_renderer_with_index_planes(renderer, cameras, 0, P, cm->ctx, nullptr));
  const int32_t* d_labels = P ? prim_labels_dev : reinterpret_cast<const int32_t*>(cm->d_counts);
  // Groups of up to eight views through the multi-view rasteriser launches of smesh_fuse_views, on the main stream: the counting
  // kernel of a view is a few microseconds, so there is nothing for a second stream to hide.
  for (uint64_t i = 0; i < n; i += 8) {
    const int m = (int)std::min<uint64_t>(8, n - i);
    bool staged = false;
    SMESH_TRY(smesh_renderer_with_index_planes(renderer, &cameras[i], m, P, cm->ctx,
                                               [&](int v, const uint32_t* d_idx, uint64_t W, uint64_t H) -> int {
      return count_plane(cm, d_idx, d_labels, P, gts[i + (uint64_t)v], gt_dtype, gt_strides, gt_mem, W, H, &staged);
    }));
    if (staged) {   // host images are consumed before the call returns
      std::lock_guard<std::recursive_mutex> lock(cm->ctx->mu);
      SMESH_HIP(hipSetDevice(cm->ctx->device));
      SMESH_HIP(hipStreamSynchronize(cm->ctx->stream));
    }
  }
  return SMESH_OK;
}

int smesh_confusion_add_view(smesh_confusion_t* cm, smesh_renderer_t* renderer, const smesh_camera_t* camera,
                             const int32_t* prim_labels_dev, uint64_t P, const void* gt, int gt_dtype, const int64_t gt_strides[2], int gt_mem) {
  if (!camera) return fail(SMESH_ERR_INVALID, "NULL argument");
  return smesh_confusion_add_views(cm, renderer, camera, 1, prim_labels_dev, P, &gt, gt_dtype, gt_strides, gt_mem);
}

}  // extern "C"
