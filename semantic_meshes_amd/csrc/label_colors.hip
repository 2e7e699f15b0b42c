// label_colors.hip -- label images that are colour images (include/smesh_label_colors.h, where the rule is stated to the bit): the
// distinct colours of images (k_colors_mark, k_colors_count, k_colors_list, smesh_colors_unique) and the dense (W,H) plane of a colour
// image and a colour table (k_labels_prepare_colors, its launcher and smesh_labels_prepare_colors).  The fusion entry points of that
// header live beside their counterparts in fusion_labels.hip and call smesh_label_colors_launch from narrow_plane().
//
// Per output pixel (X, Y):  sx = ((2X + 1) w) div (2W),  sy = ((2Y + 1) h) div (2H)   (integers; no floating point anywhere)
//                           p  = in + sx * s0 + sy * s1;   key = p[0] << 16 | p[s2] << 8 | p[2 s2]
//                           c  = classes[j] where keys[j] == key (bisection), else don't care
//                           out[X * H + Y] = c in [0, C) ? c : all ones
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "labels_scratch.hpp"
#include "../../include/smesh_label_colors.h"

#include <algorithm>
#include <atomic>
#include <mutex>

using namespace smesh;

namespace {

constexpr uint32_t kTableLdsMax = SMESH_LABEL_COLORS_LDS_MAX;   // entries of a table kept in LDS
constexpr uint32_t kChunk = 4096;                               // pixels per workgroup (one LDS table copy serves them)
constexpr uint32_t kKeyBits = 24;
constexpr uint32_t kBitmapWords = 1u << (kKeyBits - 5);         // 2^24 bits as 32-bit words: 2 MiB
constexpr uint32_t kListBlock = 256;                            // bitmap words per workgroup of k_colors_count / k_colors_list
constexpr uint32_t kListBlocks = kBitmapWords / kListBlock;     // 2048
constexpr int kGroup = 8;                                       // images whose bitmaps share a memset and a synchronisation

static_assert(kTableLdsMax * 6u <= 64u * 1024u, "the table's LDS copy must fit what a workgroup gets without asking");

std::atomic<uint64_t> g_launches{0};

// ---- distinct colours ---------------------------------------------------------------------------------------------------------
struct MarkArgs {
  const void* in;
  int64_t s0, s1, s2;   // element strides; the host orders the two image axes so that s1 <= s0 (lanes run along the closer axis)
  uint32_t w, h;
  uint32_t* bitmap;     // [kBitmapWords] of this image
};

template <typename T, int CH>
__device__ __forceinline__ uint32_t key_at(const T* __restrict__ p, int64_t s2) {
  if (CH == 1) return (uint32_t)p[0];
  return ((uint32_t)p[0] << 16) | ((uint32_t)p[s2] << 8) | (uint32_t)p[2 * s2];
}

// Bit `key` of the image's bitmap for every pixel.  Masks are large uniform regions, so nearly every pixel finds its bit set: a lane
// reads the word with a plain load and issues the atomic OR only where its bit reads 0.  A stale plain read cannot lose a colour:
// inside a launch a bit only ever goes from 0 to 1 (the memset that clears the bitmap is an earlier operation of the same stream), so
// a read that is older than the truth can only show 0 where memory holds 1 -- the lane then issues an OR that changes nothing.  A
// read never shows 1 for a bit nobody set.  The OR itself is a device-scope atomic, executed at the memory side, so no set bit is
// lost between lanes, waves or XCDs; and whoever reads the bitmap (k_colors_count, k_colors_list) is a later launch on the same
// stream, which starts after this one's memory operations are complete and visible.
// The neighbour-key shortcut: a lane whose left neighbour in the wave holds the same key leaves the test to it -- in a mask of uniform
// regions a few lanes of a wave test, the others do not even load the bitmap word.  Measured against the form without it and kept by
// the rule of tools/color_labels_bench.py: faster beyond the spread on uniform masks (the kernel 46 -> 14 us at 1024 x 512), not
// slower on random ones.  A wave-wide form (one lane per distinct key of the wave, elected in a ballot loop) lost on random masks and
// was dropped.  A lane walks its 16 pixels one after the other on purpose: a form that issued the loads of four pixels a lane
// together, with four times the workgroups, was EIGHT times slower (373 us) -- with more lanes in flight, more of them read their bit
// as 0 before the first OR lands and pile their ORs onto the same few words.
template <typename T, int CH>
__global__ __launch_bounds__(256) void k_colors_mark(MarkArgs a) {
  const T* __restrict__ in = static_cast<const T*>(a.in);
  const uint32_t N = a.w * a.h;   // (< 2^31: smesh_colors_unique refuses more, so base + k cannot wrap)
  const uint32_t base = blockIdx.x * kChunk;
  for (uint32_t k = threadIdx.x; k < kChunk; k += 256u) {
    const uint32_t i = base + k;
    if (i >= N) break;
    const uint32_t x = i / a.h, y = i - x * a.h;
    const uint32_t key = key_at<T, CH>(in + (uint64_t)x * (uint64_t)a.s0 + (uint64_t)y * (uint64_t)a.s1, a.s2);
    // (the lanes past the image's end are the wave's LAST ones: the left neighbour of an active lane is active, and lane 0, which
    // reads its own key back, always tests)
    const uint32_t left = (uint32_t)__shfl_up((int)key, 1);
    if ((threadIdx.x & 63u) != 0u && left == key) continue;
    const uint32_t word = key >> 5, bit = 1u << (key & 31u);   // key < 2^24 (three bytes, or one value of at most 16 bits): word < kBitmapWords
    if ((a.bitmap[word] & bit) == 0u) atomicOr(&a.bitmap[word], bit);
  }
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* __restrict__ sh) {
  // 256 threads: the sum of v over the workgroup, to every thread.  sh: 256 words.
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t s = 128u; s > 0u; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const uint32_t r = sh[0];
  __syncthreads();
  return r;
}

// Set bits of each run of kListBlock words: block_counts[image][block].  grid = (kListBlocks, images).
__global__ __launch_bounds__(256) void k_colors_count(const uint32_t* __restrict__ bitmaps, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t sh[256];
  const uint32_t* __restrict__ bm = bitmaps + (size_t)blockIdx.y * kBitmapWords;
  const uint32_t c = block_sum((uint32_t)__popc(bm[blockIdx.x * kListBlock + threadIdx.x]), sh);
  if (threadIdx.x == 0) block_counts[blockIdx.y * kListBlocks + blockIdx.x] = c;
}

// The ascending key list of each bitmap: a workgroup's first output position is the sum of the counts of the blocks before it, a
// word's the exclusive prefix sum of the population counts inside the block; each lane writes the keys of its word, lowest bit first.
// At most `cap` keys are written; counts[image] is always the true number.  The bitmap is only read.  grid = (kListBlocks, images).
__global__ __launch_bounds__(256) void k_colors_list(const uint32_t* __restrict__ bitmaps, const uint32_t* __restrict__ block_counts,
                                                     uint32_t* __restrict__ keys, uint32_t cap, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t sh[256];
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  const uint32_t* __restrict__ bc = block_counts + blockIdx.y * kListBlocks;
  uint32_t before = 0u;
  for (uint32_t j = t; j < b; j += 256u) before += bc[j];
  const uint32_t first = block_sum(before, sh);
  uint32_t word = bitmaps[(size_t)blockIdx.y * kBitmapWords + b * kListBlock + t];
  // inclusive scan of the population counts (Hillis-Steele over 256 entries)
  const uint32_t mine = (uint32_t)__popc(word);
  sh[t] = mine;
  __syncthreads();
  for (uint32_t s = 1u; s < 256u; s <<= 1) {
    const uint32_t add = t >= s ? sh[t - s] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  uint32_t pos = first + sh[t] - mine;
  if (b == kListBlocks - 1u && t == 255u) counts[blockIdx.y] = (unsigned long long)first + sh[t];
  uint32_t* __restrict__ out = keys + (size_t)blockIdx.y * cap;
  const uint32_t key0 = (b * kListBlock + t) << 5;
  while (word && pos < cap) {
    const uint32_t bit = (uint32_t)__ffs((int)word) - 1u;
    word &= word - 1u;
    out[pos++] = key0 + bit;
  }
}

template <typename T>
void launch_mark(int channels, const MarkArgs& a, hipStream_t st) {
  const dim3 g((uint32_t)div_up((uint64_t)a.w * a.h, kChunk)), b(256);
  if (channels == 1) hipLaunchKernelGGL((k_colors_mark<T, 1>), g, b, 0, st, a);
  else hipLaunchKernelGGL((k_colors_mark<T, 3>), g, b, 0, st, a);
}

// ---- the plane of a colour image -------------------------------------------------------------------------------------------------
struct ColorPrepArgs {
  const uint8_t* in;
  int64_t s0, s1, s2;
  uint32_t w, h, W, H;
  uint32_t C, K;
  const uint32_t* keys;      // device memory, strictly ascending
  const int32_t* classes;    // device memory
  void* out;
  uint32_t lds;              // the table is copied into LDS: keys, then narrowed 2-byte codes
};

// The rule of smesh_label_prep.h, per axis (label_prep.hip src_index).
__device__ __forceinline__ uint32_t src_index(uint32_t X, uint32_t n, uint32_t N) {
  const uint64_t num = (uint64_t)(2u * X + 1u) * n;
  if ((num >> 32) == 0) return (uint32_t)num / (2u * N);
  return (uint32_t)(num / (2ull * N));
}

// The last entry that is <= key, if any, is in [lo, lo + n): n halves until it is 1.  K >= 1, and lo + half < lo + n <= K.
__device__ __forceinline__ uint32_t bisect(const uint32_t* __restrict__ keys, uint32_t K, uint32_t key) {
  uint32_t lo = 0u, n = K;
  while (n > 1u) {
    const uint32_t half = n >> 1;
    if (keys[lo + half] <= key) lo += half;
    n -= half;
  }
  return lo;
}

template <typename OUT>
__global__ __launch_bounds__(256) void k_labels_prepare_colors(ColorPrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr OUT kDontCare = (OUT)~(OUT)0;
  uint32_t* lkeys = reinterpret_cast<uint32_t*>(smem);
  uint16_t* lcodes = reinterpret_cast<uint16_t*>(smem + (size_t)a.K * 4);
  if (a.lds) {
    for (uint32_t i = threadIdx.x; i < a.K; i += 256u) {
      const int32_t c = a.classes[i];
      lkeys[i] = a.keys[i];
      lcodes[i] = (c >= 0 && (uint32_t)c < a.C) ? (uint16_t)c : (uint16_t)0xFFFFu;   // (a uint8 plane has C <= 255: 65535 becomes 255)
    }
    __syncthreads();
  }
  OUT* __restrict__ out = static_cast<OUT*>(a.out);
  const uint32_t N = a.W * a.H;   // (< 2^29)
  const uint32_t base = blockIdx.x * kChunk;
  for (uint32_t k = threadIdx.x; k < kChunk; k += 256u) {
    const uint32_t i = base + k;
    if (i >= N) break;
    const uint32_t X = i / a.H, Y = i - X * a.H;
    const uint64_t sx = src_index(X, a.w, a.W), sy = src_index(Y, a.h, a.H);
    const uint32_t key = key_at<uint8_t, 3>(a.in + sx * (uint64_t)a.s0 + sy * (uint64_t)a.s1, a.s2);
    OUT code = kDontCare;
    if (a.lds) {
      const uint32_t j = bisect(lkeys, a.K, key);
      if (lkeys[j] == key) code = (OUT)lcodes[j];
    } else {
      const uint32_t j = bisect(a.keys, a.K, key);
      if (a.keys[j] == key) {
        const int32_t c = a.classes[j];
        if (c >= 0 && (uint32_t)c < a.C) code = (OUT)c;
      }
    }
    out[i] = code;
  }
}

int check_table(const uint32_t* keys, const int32_t* classes, uint64_t K) {
  if (!keys || !classes) return fail(SMESH_ERR_INVALID, "colour table is NULL");
  if (K == 0) return fail(SMESH_ERR_INVALID, "colour table is empty");
  if (K > (1ull << kKeyBits)) return fail(SMESH_ERR_INVALID, "colour table has more than 2^24 entries");
  for (uint64_t j = 0; j < K; j++) {
    if (keys[j] >> kKeyBits) return fail(SMESH_ERR_INVALID, "colour table: a key is not below 2^24");
    if (j && keys[j] <= keys[j - 1]) return fail(SMESH_ERR_INVALID, "colour table: keys must be strictly ascending");
  }
  return SMESH_OK;
}

// bytes from the first to the last element read of a (w,h,3) uint8 image (a fourth channel is never read)
size_t color_span(const int64_t s[3], uint64_t w, uint64_t h, int channels, size_t item) {
  return (size_t)(1 + (w - 1) * (uint64_t)s[0] + (h - 1) * (uint64_t)s[1] + (channels == 1 ? 0 : 2 * (uint64_t)s[2])) * item;
}

}  // namespace

// (context.cpp: the read-only option "labels_colors_launches")
namespace smesh {
uint64_t smesh_label_colors_launches() { return g_launches.load(); }
}  // namespace smesh

int smesh_label_colors_check(int dt, const int64_t* strides, const LabelPrep& p) {
  if (p.channels != 3 && p.channels != 4) return fail(SMESH_ERR_INVALID, "a colour image has 3 or 4 channels");
  if (dt != SMESH_LBL_U8) return fail(SMESH_ERR_INVALID, "a colour image is uint8");
  if (strides && (strides[0] < 0 || strides[1] < 0 || strides[2] < 0)) return fail(SMESH_ERR_INVALID, "labels: negative strides are not supported");
  return check_table(p.keys, p.classes, p.table_len);
}

int smesh_label_colors_launch(DeviceCtx* ctx, const void* src, const int64_t* strides, uint64_t w, uint64_t h, const uint32_t* keys_dev,
                              const int32_t* classes_dev, uint64_t K, uint32_t C, void* out, int out_bytes, uint64_t W, uint64_t H) {
  if (W == 0 || H == 0) return SMESH_OK;
  ColorPrepArgs a;
  a.in = static_cast<const uint8_t*>(src);
  a.s0 = strides[0]; a.s1 = strides[1]; a.s2 = strides[2];
  a.w = (uint32_t)w; a.h = (uint32_t)h; a.W = (uint32_t)W; a.H = (uint32_t)H;
  a.C = C;
  a.K = (uint32_t)K;
  a.keys = keys_dev;
  a.classes = classes_dev;
  a.out = out;
  a.lds = K <= kTableLdsMax ? 1u : 0u;
  const dim3 g((uint32_t)div_up(W * H, kChunk)), b(256);
  const size_t lds = a.lds ? (size_t)K * 6 : 0;
  if (out_bytes == 1) hipLaunchKernelGGL((k_labels_prepare_colors<uint8_t>), g, b, lds, ctx->stream, a);
  else hipLaunchKernelGGL((k_labels_prepare_colors<uint16_t>), g, b, lds, ctx->stream, a);
  SMESH_HIP(hipGetLastError());
  g_launches.fetch_add(1);
  return SMESH_OK;
}

extern "C" int smesh_labels_prepare_colors(const void* in, int channels, const int64_t in_strides[3], int in_memkind, uint64_t w, uint64_t h,
                                           const uint32_t* keys, const int32_t* classes, uint64_t K, uint32_t C, void* out, int out_dtype,
                                           uint64_t W, uint64_t H, int device) {
  LabelPrep p{w, h, nullptr, 0, SMESH_MEM_HOST};
  p.channels = channels; p.keys = keys; p.classes = classes; p.table_len = K;
  SMESH_TRY(smesh_label_colors_check(SMESH_LBL_U8, in_strides, p));
  SMESH_TRY(smesh_label_prep_check(SMESH_LBL_U8, in_strides, in_memkind, p, W, H, C));
  if (out_dtype != SMESH_LBL_U8 && out_dtype != SMESH_LBL_U16) return fail(SMESH_ERR_INVALID, "a prepared plane is uint8 or uint16");
  if (C == 0 || (out_dtype == SMESH_LBL_U8 && C > 255u)) return fail(SMESH_ERR_INVALID, "a uint8 plane holds 1 to 255 classes, a uint16 plane up to 65535");
  if (W == 0 || H == 0) return SMESH_OK;
  if (!in || !out) return fail(SMESH_ERR_INVALID, "NULL argument");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const int64_t dense[3] = {(int64_t)h * channels, channels, 1};
  const int64_t* s = in_strides ? in_strides : dense;
  const size_t span = color_span(s, w, h, channels, 1);
  const size_t span_al = (span + 255) & ~(size_t)255;
  const bool stage_in = in_memkind == SMESH_MEM_HOST;
  char* tmp = nullptr;   // [the staged keys][the staged classes][the staged source]
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&tmp), K * 8 + (stage_in ? span_al : 0) + 256));
  int status = SMESH_OK;
  hipError_t e = hipMemcpyAsync(tmp, keys, K * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + K * 4, classes, K * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && stage_in) {
    char* d = tmp + K * 8;
    e = hipMemcpyAsync(d, in, span, hipMemcpyHostToDevice, ctx->stream);
    in = d;
  }
  if (e == hipSuccess)
    status = smesh_label_colors_launch(ctx, in, s, w, h, reinterpret_cast<const uint32_t*>(tmp), reinterpret_cast<const int32_t*>(tmp + K * 4), K, C, out,
                                       out_dtype == SMESH_LBL_U8 ? 1 : 2, W, H);
  if (e == hipSuccess && status == SMESH_OK) e = hipStreamSynchronize(ctx->stream);
  (void)dev_free(tmp);
  SMESH_HIP(e);
  return status;
}

extern "C" int smesh_colors_unique(const void* const* images, uint64_t n, int channels, int dtype, const int64_t strides[3], int memkind,
                                   uint64_t w, uint64_t h, uint32_t* keys_out, uint64_t cap, uint64_t* counts_out, int device) {
  if (channels != 1 && channels != 3 && channels != 4) return fail(SMESH_ERR_INVALID, "an image of colours has 1, 3 or 4 channels");
  if (dtype != SMESH_LBL_U8 && !(channels == 1 && dtype == SMESH_LBL_U16))
    return fail(SMESH_ERR_INVALID, "an image of colours is uint8 (uint16 too with one channel)");
  if (strides && (strides[0] < 0 || strides[1] < 0 || (channels != 1 && strides[2] < 0)))
    return fail(SMESH_ERR_INVALID, "labels: negative strides are not supported");
  if (memkind != SMESH_MEM_HOST && memkind != SMESH_MEM_DEVICE) return fail(SMESH_ERR_INVALID, "bad memory kind");
  if (w > 65536 || h > 65536 || w * h >= (1ull << 31)) return fail(SMESH_ERR_INVALID, "image too large: at most 65536 pixels a side and fewer than 2^31 pixels");
  if (n && (!images || !counts_out || (cap && !keys_out))) return fail(SMESH_ERR_INVALID, "NULL argument");
  for (uint64_t i = 0; i < n; i++)
    if (!images[i] && w && h) return fail(SMESH_ERR_INVALID, "NULL image");
  if (n == 0) return SMESH_OK;
  if (w == 0 || h == 0) {
    for (uint64_t i = 0; i < n; i++) counts_out[i] = 0;
    return SMESH_OK;
  }
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  const size_t item = dtype == SMESH_LBL_U16 ? 2 : 1;
  const int64_t dense[3] = {(int64_t)h * channels, channels, 1};
  int64_t s[3] = {strides ? strides[0] : dense[0], strides ? strides[1] : dense[1], (strides && channels != 1) ? strides[2] : 1};
  const size_t span = color_span(s, w, h, channels, item);
  const size_t span_al = (span + 255) & ~(size_t)255;
  // the marking is indifferent to the order of the pixels: lanes run along the image axis with the smaller stride
  uint64_t mw = w, mh = h;
  if (s[0] < s[1]) { std::swap(s[0], s[1]); std::swap(mw, mh); }
  const uint32_t dcap = (uint32_t)std::min<uint64_t>(cap, 1ull << kKeyBits);   // (an image has at most 2^24 distinct keys)
  const int m_max = (int)std::min<uint64_t>(kGroup, n);
  const bool stage = memkind == SMESH_MEM_HOST;
  // [bitmaps][block counts][counts][keys][staged images]
  const size_t bm_bytes = (size_t)kBitmapWords * 4, bc_bytes = (size_t)kListBlocks * 4;
  const size_t keys_bytes = ((size_t)dcap * 4 + 255) & ~(size_t)255;
  char* tmp = nullptr;
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&tmp), (bm_bytes + bc_bytes + 256 + keys_bytes + (stage ? span_al : 0)) * (size_t)m_max));
  uint32_t* d_bm = reinterpret_cast<uint32_t*>(tmp);
  uint32_t* d_bc = reinterpret_cast<uint32_t*>(tmp + bm_bytes * m_max);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(tmp + (bm_bytes + bc_bytes) * m_max);
  uint32_t* d_keys = reinterpret_cast<uint32_t*>(tmp + (bm_bytes + bc_bytes + 256) * m_max);
  char* d_stage = tmp + (bm_bytes + bc_bytes + 256 + keys_bytes) * m_max;
  hipError_t e = hipSuccess;
  for (uint64_t i = 0; i < n && e == hipSuccess; i += kGroup) {
    const int m = (int)std::min<uint64_t>(kGroup, n - i);
    e = hipMemsetAsync(d_bm, 0, bm_bytes * (size_t)m, ctx->stream);
    for (int v = 0; v < m && e == hipSuccess; v++) {
      const void* src = images[i + v];
      if (stage) {
        char* d = d_stage + (size_t)v * span_al;
        e = hipMemcpyAsync(d, src, span, hipMemcpyHostToDevice, ctx->stream);
        src = d;
      }
      if (e != hipSuccess) break;
      const MarkArgs a{src, s[0], s[1], s[2], (uint32_t)mw, (uint32_t)mh, d_bm + (size_t)v * kBitmapWords};
      if (item == 2) launch_mark<uint16_t>(channels, a, ctx->stream);
      else launch_mark<uint8_t>(channels, a, ctx->stream);
      e = hipGetLastError();
    }
    if (e != hipSuccess) break;
    const dim3 g(kListBlocks, (uint32_t)m), b(256);
    hipLaunchKernelGGL(k_colors_count, g, b, 0, ctx->stream, d_bm, d_bc);
    // (the keys of image v start at d_keys + v * dcap: k_colors_list's row pitch is the capacity itself)
    hipLaunchKernelGGL(k_colors_list, g, b, 0, ctx->stream, d_bm, d_bc, d_keys, dcap, d_counts);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(counts_out + i, d_counts, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && dcap) {
      if (dcap == cap) e = hipMemcpyAsync(keys_out + i * cap, d_keys, (size_t)m * dcap * 4, hipMemcpyDeviceToHost, ctx->stream);
      else e = hipMemcpy2DAsync(keys_out + i * cap, cap * 4, d_keys, (size_t)dcap * 4, (size_t)dcap * 4, (size_t)m, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // once per group: the results are on the host, the scratch is free
  }
  (void)dev_free(tmp);
  SMESH_HIP(e);
  return SMESH_OK;
}
