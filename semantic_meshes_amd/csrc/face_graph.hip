// face_graph.hip -- mesh-graph operations (include/smesh_face_graph.h): the faces across every face's edges as a CSR built on the
// device from the vertex-to-faces CSR of vertices.hip, T averaging iterations over it (smooth or fill), and per-entry weights
// from the agreement of the two faces' normals.
//
// The reference has no such step.  Graph, propagation and weights are defined to the bit in the header: every face (graph) and
// every (face, class) element (propagation) is owned by ONE lane that adds in list order, so there are no float atomics, and the
// launch boundary is the only synchronisation between two iterations.
#include "mesh_host.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smesh_face_graph.h"

using namespace smesh;

struct smesh_face_graph {
  DeviceCtx* ctx = nullptr;
  uint64_t F = 0, V = 0, nnz = 0;
  uint32_t* offsets = nullptr;      // [F + 1]
  uint32_t* neighbours = nullptr;   // [nnz] the list of face f: neighbours[offsets[f] .. offsets[f + 1])
};

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;

#include "scan.inc.hpp"   // k_scan_tiles, k_scan_sums, k_scan_add

// ---- building the CSR ----------------------------------------------------------------------------------------------------------
// One thread owns face f: for each of its edge slots it walks the shorter of the two vertices' ascending face lists (voff, vlist:
// the vertex map) and keeps the faces that name the other vertex.  !FILL: out[f] = the number of entries, and their sum over all
// faces in *total (integer atomics, one per wave: it only guards the 2^32 limit).  FILL: out[offsets[f] ..] = the entries.
// A hub vertex with thousands of faces makes this one thread's walk long (smesh_face_graph.h).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_fg_walk(const int32_t* __restrict__ faces, uint64_t F, const uint32_t* __restrict__ voff,
                                                    const uint32_t* __restrict__ vlist, const uint32_t* __restrict__ offsets,
                                                    uint32_t* __restrict__ out, unsigned long long* __restrict__ total) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t n = 0;
  if (f < F) {
    const int v[3] = {faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2]};
    const uint32_t base = FILL ? offsets[f] : 0u;
    for (int s = 0; s < 3; s++) {
      const int a = v[s], b = v[(s + 1) % 3];
      if (a == b) continue;
      bool again = false;      // the same unordered pair as an earlier slot
      for (int e = 0; e < s; e++) {
        const int pa = v[e], pb = v[(e + 1) % 3];
        again = again || (pa == a && pb == b) || (pa == b && pb == a);
      }
      if (again) continue;
      const uint32_t ba = voff[a], na = voff[a + 1] - ba, bb = voff[b], nb = voff[b + 1] - bb;
      const bool walk_a = na <= nb;
      const uint32_t beg = walk_a ? ba : bb, len = walk_a ? na : nb;
      const int other = walk_a ? b : a;
      for (uint32_t k = beg; k < beg + len; k++) {
        const uint32_t g = vlist[k];
        if (g == (uint32_t)f) continue;
        const int32_t* const gv = faces + (uint64_t)g * 3;
        if (gv[0] == other || gv[1] == other || gv[2] == other) {
          if (FILL) out[base + n] = g;
          n++;
        }
      }
    }
    if (!FILL) out[f] = n;
  }
  if (!FILL) {
    unsigned long long sum = n;
    for (int d = kWave >> 1; d > 0; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && sum) atomicAdd(total, sum);
  }
}

// ---- the propagation -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_face_unreached(const float* __restrict__ tot, uint64_t F, unsigned long long* __restrict__ count) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool un = f < F && !(tot[f] > 0.0f);
  const unsigned long long mask = __ballot(un);
  if ((threadIdx.x & (kWave - 1)) == 0 && mask) atomicAdd(count, (unsigned long long)__popcll(mask));
}

constexpr int kModeTotals = 2;   // beside SMESH_FG_SMOOTH and SMESH_FG_FILL: no walk, nothing written but totn = the totals of x0

struct PropArgs {
  const uint32_t* offsets;   // [F + 1]
  const uint32_t* nbr;       // [nnz]
  const float* w;            // [nnz] or null
  const float* x0;           // [F, C] the source: never written
  const float* xt;           // [F, C] x_t (x0 itself at t == 0)
  const float* tot0;         // [F] row totals of x0
  const float* tott;         // [F] row totals of x_t
  float* xn;                 // [F, C] x_{t+1}
  float* totn;               // [F] its row totals
  uint64_t F;
  uint32_t C;
  int mode;
  float alpha, om, observed;
};

// The value of lane `src` of the wave; a group of one lane reads itself.
template <int G, typename T>
__device__ __forceinline__ T group_read(T v, int src) {
  if (G == 1) return v;
  return __shfl(v, src, kWave);
}

// One iteration, in the shape of k_vertex_gather (vertices.hip): a group of G lanes owns one face; lane l of the group owns the
// classes l, l + G, ... (NCH of them, in registers).  Rows of up to 64 classes take groups of 4 or 8 lanes -- 16 or 8 faces per wave:
// measured against groups of 16, 32 and 64 lanes, the narrower group won at 19 and at 40 classes because a wave then has more
// rows in flight.  Wider rows take a wave per face and walk the classes in coalesced chunks of 64, up to
// kMaxRegisterChunks of them; NCH == 0: any class count, chunk after chunk, the list walked once per chunk.  Neighbour ids, weights
// and neighbour totals are read once per group -- lane l reads entry l of each run of G entries, the others get it by a cross-lane
// read -- and up to four neighbour rows are in flight, added one after another in list order.  The new row's total is added in
// ascending class order by the group's first lane, from the group's elements laid side by side in LDS (k_vertex_gather's serial
// cross-lane reads cost more: measured).  mode kModeTotals: the same total step on x0 alone, which is how tot_0 is made.
template <int G, int NCH>
__global__ __launch_bounds__(kBlock) void k_face_propagate(PropArgs a) {
  constexpr int R = NCH > 0 ? NCH : 1;
  constexpr bool LT = G >= 4;             // the row total through LDS; groups of one or two lanes add their one or two elements directly
  __shared__ float lds[LT ? kBlock * R : 1];     // LT: per wave 64 R floats, a group's new elements side by side
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t f = tid / G;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int gl = lane & (G - 1);          // lane within the group
  const int gbase = lane - gl;            // first lane of the group within the wave
  const bool valid = f < a.F;             // (a whole group at a time: nobody leaves before the cross-lane steps)
  const uint32_t C = a.C;
  const bool weighted = a.w != nullptr;

  uint32_t beg = 0, end = 0;
  const bool totals_only = a.mode == kModeTotals;
  bool keep = false;                      // FILL: an observed face keeps x0 and needs no walk; nor does a launch for x0's totals
  if (valid) {
    keep = totals_only || (a.mode == SMESH_FG_FILL && a.tot0[f] >= a.observed);
    if (!keep) { beg = a.offsets[f]; end = a.offsets[f + 1]; }
  }
  const float* const xt = a.xt;
  const uint32_t chunks = NCH > 0 ? (uint32_t)NCH : (C + G - 1) / G;

  float total = 0.0f;                     // the new row's total, added in ascending c (LT: in the group's first lane only)
  float s[R], own[R];
  for (uint32_t ch0 = 0; ch0 < chunks; ch0 += R) {
#pragma unroll
    for (int j = 0; j < R; j++) {         // the face's own elements: asked for before the walk, needed after it
      const uint32_t c = (ch0 + j) * G + gl;
      s[j] = 0.0f;
      own[j] = valid && c < C ? a.x0[f * C + c] : 0.0f;
    }
    float dw = 0.0f;                      // the sum of the informed entries' weights, in list order
    uint32_t dn = 0;                      // the number of informed entries
    for (uint32_t run = beg; run < end; run += G) {
      const uint32_t k = run + (uint32_t)gl;
      const bool has = k < end;
      const uint32_t my_g = has ? a.nbr[k] : 0u;
      const int my_inf = has && a.tott[my_g] > 0.0f ? 1 : 0;
      const float my_w = has && weighted ? a.w[k] : 0.0f;
      const int n = (int)min((uint32_t)G, end - run);
      for (int e0 = 0; e0 < n; e0 += 4) {
        uint64_t g[4];
        bool inf[4];
        float wk[4], x[4][R];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int src = gbase + ((e0 + i) & (G - 1));
          g[i] = group_read<G>(my_g, src);
          inf[i] = group_read<G>(my_inf, src) != 0 && e0 + i < n;
          wk[i] = group_read<G>(my_w, src);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
          for (int j = 0; j < R; j++) {
            const uint32_t c = (ch0 + j) * G + gl;
            x[i][j] = inf[i] && c < C ? xt[g[i] * C + c] : 0.0f;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if (inf[i]) {
            if (weighted) {
#pragma unroll
              for (int j = 0; j < R; j++) s[j] = s[j] + wk[i] * x[i][j];
              dw = dw + wk[i];
            } else {
#pragma unroll
              for (int j = 0; j < R; j++) s[j] = s[j] + x[i][j];
              dn++;
            }
          }
        }
      }
    }
    const float d = weighted ? dw : (float)dn;
    // the new elements, then their total in ascending class order
    float r[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
      const uint32_t c = (ch0 + j) * G + gl;
      r[j] = 0.0f;
      if (valid && c < C) {
        if (a.mode == SMESH_FG_SMOOTH) r[j] = d > 0.0f ? a.om * own[j] + a.alpha * (s[j] / d) : own[j];
        else r[j] = keep ? own[j] : d > 0.0f ? s[j] / d : xt[f * C + c];
        if (!totals_only) a.xn[f * C + c] = r[j];
      }
    }
    if (LT) {
      // through LDS: the group's elements side by side, then its first lane adds them one after another (the lanes of a wave run
      // in lockstep and its LDS accesses complete in order: no barrier beyond the compiler's)
      float* const mine = lds + (threadIdx.x & ~(kWave - 1)) * R + gbase * R;
#pragma unroll
      for (int j = 0; j < R; j++) mine[j * G + gl] = r[j];
      __builtin_amdgcn_wave_barrier();
      const uint32_t c0 = ch0 * G;
      const int n = (int)min((uint32_t)(G * R), C > c0 ? C - c0 : 0u);
      if (gl == 0) {
        int l = 0;
        if ((G * R) % 4 == 0) {
          for (; l + 4 <= n; l += 4) {
            const float4 v = *reinterpret_cast<const float4*>(mine + l);
            total += v.x; total += v.y; total += v.z; total += v.w;
          }
        }
        for (; l < n; l++) total += mine[l];
      }
      __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
      for (int j = 0; j < R; j++) {
        const uint32_t c0 = (ch0 + j) * G;
        const int width = (int)min((uint32_t)G, C > c0 ? C - c0 : 0u);
        if (G == 1) {
          if (width) total += r[j];
        } else {
          for (int l = 0; l < width; l++) total += __shfl(r[j], gbase + l, kWave);
        }
      }
    }
  }
  if (valid && gl == 0) a.totn[f] = total;
}

template <int G, int NCH>
void launch_one(const PropArgs& a, hipStream_t st) {
  const uint64_t threads = a.F * G;
  hipLaunchKernelGGL((k_face_propagate<G, NCH>), dim3((uint32_t)div_up(threads, kBlock)), dim3(kBlock), 0, st, a);
}

constexpr uint32_t kMaxRegisterChunks = 8;   // rows of up to 512 classes keep their sums in registers

// Groups of 4 lanes up to 32 classes, of 8 lanes up to 64, a wave beyond: the narrowest group whose lanes hold at most
// kMaxRegisterChunks classes each, because what a narrower group buys is more faces -- more rows in flight -- per wave.
void launch_propagate(const PropArgs& a, hipStream_t st) {
  const uint32_t C = a.C;
  if (C <= 1) launch_one<1, 1>(a, st);
  else if (C <= 2) launch_one<2, 1>(a, st);
  else if (C <= 32) {
    switch (div_up(C, 4)) {
      case 1: launch_one<4, 1>(a, st); break;
      case 2: launch_one<4, 2>(a, st); break;
      case 3: launch_one<4, 3>(a, st); break;
      case 4: launch_one<4, 4>(a, st); break;
      case 5: launch_one<4, 5>(a, st); break;
      case 6: launch_one<4, 6>(a, st); break;
      case 7: launch_one<4, 7>(a, st); break;
      default: launch_one<4, 8>(a, st); break;
    }
  } else if (C <= 64) {
    switch (div_up(C, 8)) {
      case 5: launch_one<8, 5>(a, st); break;
      case 6: launch_one<8, 6>(a, st); break;
      case 7: launch_one<8, 7>(a, st); break;
      default: launch_one<8, 8>(a, st); break;
    }
  } else {
    switch (div_up(C, kWave) <= kMaxRegisterChunks ? (int)div_up(C, kWave) : 0) {
      case 2: launch_one<kWave, 2>(a, st); break;
      case 3: launch_one<kWave, 3>(a, st); break;
      case 4: launch_one<kWave, 4>(a, st); break;
      case 5: launch_one<kWave, 5>(a, st); break;
      case 6: launch_one<kWave, 6>(a, st); break;
      case 7: launch_one<kWave, 7>(a, st); break;
      case 8: launch_one<kWave, 8>(a, st); break;
      default: launch_one<kWave, 0>(a, st); break;
    }
  }
}

// ---- the normal weights --------------------------------------------------------------------------------------------------------
// nl[f] = (nx, ny, nz, l) of face f by the header's rule; *bad is set by a face index outside [0, V).
__global__ __launch_bounds__(kBlock) void k_fg_normals(const int32_t* __restrict__ faces, uint64_t F, uint64_t V, const float* __restrict__ vertices,
                                                       float4* __restrict__ nl, uint32_t* __restrict__ bad) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || (uint64_t)i0 >= V || (uint64_t)i1 >= V || (uint64_t)i2 >= V) {
    atomicOr(bad, 1u);
    nl[f] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float* const p0 = vertices + (uint64_t)i0 * 3;
  const float* const p1 = vertices + (uint64_t)i1 * 3;
  const float* const p2 = vertices + (uint64_t)i2 * 3;
  const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  nl[f] = make_float4(nx, ny, nz, sqrtf((nx * nx + ny * ny) + nz * nz));
}

// One thread owns the entries of face f.
__global__ __launch_bounds__(kBlock) void k_fg_weights(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nbr, uint64_t F,
                                                       const float4* __restrict__ nl, uint32_t power, int two_sided, float* __restrict__ w) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const float4 nf = nl[f];
  for (uint32_t k = offsets[f]; k < offsets[f + 1]; k++) {
    const float4 ng = nl[nbr[k]];
    float q = ((nf.x * ng.x + nf.y * ng.y) + nf.z * ng.z) / (nf.w * ng.w);
    if (two_sided) q = fabsf(q);
    if (!(q > 0.0f)) q = 0.0f;
    if (q > 1.0f) q = 1.0f;
    float p = q;
    for (uint32_t i = 1; i < power; i++) p = p * q;
    w[k] = p;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
int build_graph(smesh_face_graph* gr, const int32_t* faces) {
  DeviceCtx* ctx = gr->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t F = gr->F, n = F + 1;
  // the vertex-to-faces CSR: the vertex map of vertices.hip, which also refuses a face index outside [0, V)
  smesh_vertex_map_t* map = nullptr;
  SMESH_TRY(smesh_vertex_map_create(faces, F, gr->V, ctx->device, &map));
  struct MapGuard {
    smesh_vertex_map_t* m;
    ~MapGuard() { (void)smesh_vertex_map_destroy(m); }
  } guard{map};
  DeviceCtx* mctx = nullptr;
  const uint32_t *voff = nullptr, *vlist = nullptr;
  SMESH_TRY(smesh_vertex_map_tables(map, &mctx, &voff, &vlist));

  TempBlocks tmp;
  int32_t* d_faces = nullptr;
  uint32_t *count = nullptr, *tiles = nullptr;
  unsigned long long* total = nullptr;
  SMESH_TRY(tmp.alloc(&d_faces, F * 12));
  SMESH_TRY(tmp.alloc(&count, n * 4));
  SMESH_TRY(tmp.alloc(&tiles, div_up(n, kScanTile) * 4));
  SMESH_TRY(tmp.alloc(&total, 16));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&gr->offsets), std::max<uint64_t>(n * 4, 16)));
  SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));
  SMESH_HIP(hipMemsetAsync(total, 0, 16, st));
  const dim3 gf((uint32_t)div_up(F, kBlock)), b(kBlock);
  if (F) {
    SMESH_HIP(hipMemcpyAsync(d_faces, faces, F * 12, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fg_walk<false>, gf, b, 0, st, d_faces, F, voff, vlist, (const uint32_t*)nullptr, count, total);
  }
  // offsets = exclusive scan of count[0 .. F] (count[F] == 0, so offsets[F] is the number of entries)
  launch_exclusive_scan(count, gr->offsets, n, tiles, st);
  SMESH_HIP(hipGetLastError());
  unsigned long long h_total = 0;
  SMESH_HIP(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (h_total >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "face graph: the number of entries must stay below 2^32");
  gr->nnz = h_total;
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&gr->neighbours), std::max<uint64_t>(gr->nnz * 4, 16)));
  if (F && gr->nnz) {
    hipLaunchKernelGGL(k_fg_walk<true>, gf, b, 0, st, d_faces, F, voff, vlist, (const uint32_t*)gr->offsets, gr->neighbours,
                       (unsigned long long*)nullptr);
    SMESH_HIP(hipGetLastError());
  }
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

struct PropCall {
  const float* weights;
  int weights_memkind, mode;
  uint32_t iterations;
  float alpha, observed;
  int out_mode;
  float dont_care;
  float* out_rows;
  int32_t* out_labels;
  uint64_t* out_unreached;
  int out_memkind;
};

int check_prop_call(const PropCall& p) {
  if (p.mode != SMESH_FG_SMOOTH && p.mode != SMESH_FG_FILL) return fail(SMESH_ERR_INVALID, "face propagate: mode must be SMESH_FG_SMOOTH or SMESH_FG_FILL");
  if (p.mode == SMESH_FG_SMOOTH && !(p.alpha >= 0.0f && p.alpha <= 1.0f)) return fail(SMESH_ERR_INVALID, "face propagate: alpha must lie in [0, 1]");
  if (p.out_mode != SMESH_VTX_SUMS && p.out_mode != SMESH_VTX_ANNOTATIONS)
    return fail(SMESH_ERR_INVALID, "face propagate: out_mode must be SMESH_VTX_SUMS or SMESH_VTX_ANNOTATIONS");
  if (!p.out_rows && !p.out_labels) return fail(SMESH_ERR_INVALID, "face propagate: at least one of out_rows and out_labels is required");
  if (!memkind_ok(p.out_memkind) || (p.weights && !memkind_ok(p.weights_memkind))) return fail(SMESH_ERR_INVALID, "face propagate: bad memory kind");
  return SMESH_OK;
}

// The propagation over rows that are on the device already.  Context locked, device current.
int propagate_device_rows(const smesh_face_graph* gr, DeviceCtx* ctx, const float* d_x0, uint32_t C, const PropCall& p) {
  if (C == 0) return fail(SMESH_ERR_INVALID, "face propagate: the class count must be positive");
  hipStream_t st = ctx->stream;
  const uint64_t F = gr->F;
  TempBlocks tmp;
  const float* x_final = d_x0;
  float* tot_final = nullptr;
  const dim3 gf((uint32_t)div_up(F, kBlock)), b(kBlock);
  const bool need_totals = p.iterations > 0 || p.out_unreached != nullptr;
  if (F && need_totals) {
    PropArgs a = {};
    a.offsets = gr->offsets;
    a.nbr = gr->neighbours;
    SMESH_TRY(on_device(ctx, tmp, p.weights, p.weights ? gr->nnz * 4 : 0, p.weights_memkind, &a.w));
    a.x0 = d_x0;
    a.F = F;
    a.C = C;
    a.mode = p.mode;
    a.alpha = p.alpha;
    a.om = 1.0f - p.alpha;
    a.observed = p.observed;
    // x0's totals and two ping-pong pairs (rows, totals); a call of one iteration needs one pair
    float *tot0 = nullptr, *rows[2] = {nullptr, nullptr}, *tots[2] = {nullptr, nullptr};
    SMESH_TRY(tmp.alloc(&tot0, F * 4));
    for (uint32_t i = 0; i < std::min<uint32_t>(p.iterations, 2); i++) {
      SMESH_TRY(tmp.alloc(&rows[i], (size_t)F * C * 4));
      SMESH_TRY(tmp.alloc(&tots[i], F * 4));
    }
    a.mode = kModeTotals;      // tot_0: the kernel's own total step on x0
    a.totn = tot0;
    launch_propagate(a, st);
    a.mode = p.mode;
    a.tot0 = tot0;
    a.xt = d_x0;
    a.tott = tot0;
    tot_final = tot0;
    for (uint32_t t = 0; t < p.iterations; t++) {
      a.xn = rows[t & 1];
      a.totn = tots[t & 1];
      launch_propagate(a, st);
      a.xt = a.xn;
      a.tott = a.totn;
      x_final = a.xn;
      tot_final = a.totn;
    }
    SMESH_HIP(hipGetLastError());
  }
  if (p.out_unreached) {
    *p.out_unreached = 0;
    if (F) {
      unsigned long long* d_count = nullptr;
      SMESH_TRY(tmp.alloc(&d_count, 16));
      SMESH_HIP(hipMemsetAsync(d_count, 0, 16, st));
      hipLaunchKernelGGL(k_face_unreached, gf, b, 0, st, (const float*)tot_final, F, d_count);
      SMESH_HIP(hipGetLastError());
      unsigned long long h = 0;
      SMESH_HIP(hipMemcpyAsync(&h, d_count, 8, hipMemcpyDeviceToHost, st));
      SMESH_HIP(hipStreamSynchronize(st));
      *p.out_unreached = h;
    }
  }
  // the finishing step: x_T as a vertex row (k_vertex_gather, item i owns row i); it waits for the stream
  return smesh_rows_finish(ctx, x_final, F, C, p.out_mode, p.dont_care, p.out_rows, p.out_labels, p.out_memkind);
}

}  // namespace

int smesh_face_graph_tables(const smesh_face_graph* gr, DeviceCtx** ctx, const uint32_t** offsets, const uint32_t** neighbours, uint64_t* F,
                            uint64_t* nnz) {
  if (!gr) return fail(SMESH_ERR_INVALID, "NULL face graph");
  *ctx = gr->ctx;
  *offsets = gr->offsets;
  *neighbours = gr->neighbours;
  *F = gr->F;
  *nnz = gr->nnz;
  return SMESH_OK;
}

extern "C" {

int smesh_face_graph_create(const int32_t* faces, uint64_t F, uint64_t V, int device, smesh_face_graph_t** out) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (F && !faces) return fail(SMESH_ERR_INVALID, "face graph: NULL faces");
  if (3 * F >= 0xFFFFFFFFull || V >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "face graph: 3 F and V must stay below 2^32");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  smesh_face_graph* gr = new smesh_face_graph;
  gr->ctx = ctx;
  gr->F = F;
  gr->V = V;
  const int status = build_graph(gr, faces);
  if (status != SMESH_OK) {
    smesh_face_graph_destroy(gr);
    return status;
  }
  *out = gr;
  return SMESH_OK;
}

int smesh_face_graph_destroy(smesh_face_graph_t* gr) {
  if (!gr) return SMESH_OK;
  std::lock_guard<std::recursive_mutex> lock(gr->ctx->mu);
  DeviceScope scope(gr->ctx->device);
  if (gr->offsets) (void)dev_free(gr->offsets);
  if (gr->neighbours) (void)dev_free(gr->neighbours);
  delete gr;
  return SMESH_OK;
}

int smesh_face_graph_size(const smesh_face_graph_t* gr, uint64_t* F, uint64_t* V, uint64_t* nnz) {
  if (!gr) return fail(SMESH_ERR_INVALID, "NULL face graph");
  if (F) *F = gr->F;
  if (V) *V = gr->V;
  if (nnz) *nnz = gr->nnz;
  return SMESH_OK;
}

int smesh_face_graph_adjacency(const smesh_face_graph_t* gr, uint64_t* offsets, uint32_t* neighbours) {
  if (!gr || !offsets || (gr->nnz && !neighbours)) return fail(SMESH_ERR_INVALID, "NULL argument");
  return csr_to_host(gr->ctx, gr->offsets, gr->F, gr->neighbours, gr->nnz, offsets, neighbours);
}

int smesh_face_graph_propagate(const smesh_face_graph_t* gr, const float* face_rows, int rows_memkind, uint32_t C, const float* weights,
                               int weights_memkind, int mode, uint32_t iterations, float alpha, float observed_threshold, int out_mode,
                               float dont_care_threshold, float* out_rows, int32_t* out_labels, uint64_t* out_unreached, int out_memkind) {
  if (!gr) return fail(SMESH_ERR_INVALID, "NULL face graph");
  const PropCall p = {weights, weights_memkind, mode, iterations, alpha, observed_threshold, out_mode, dont_care_threshold,
                      out_rows, out_labels, out_unreached, out_memkind};
  SMESH_TRY(check_prop_call(p));
  if (C == 0) return fail(SMESH_ERR_INVALID, "face propagate: the class count must be positive");
  if (!memkind_ok(rows_memkind)) return fail(SMESH_ERR_INVALID, "face propagate: bad memory kind");
  if (gr->F && !face_rows) return fail(SMESH_ERR_INVALID, "face propagate: NULL face rows");
  DeviceCtx* ctx = gr->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(ctx, tmp, face_rows, (size_t)gr->F * C * 4, rows_memkind, &d_rows));
  return propagate_device_rows(gr, ctx, d_rows, C, p);
}

int smesh_aggregator_face_propagate(smesh_aggregator_t* ag, const smesh_face_graph_t* gr, const float* weights, int weights_memkind, int mode,
                                    uint32_t iterations, float alpha, float observed_threshold, int out_mode, float dont_care_threshold,
                                    float* out_rows, int32_t* out_labels, uint64_t* out_unreached, int out_memkind) {
  if (!ag || !gr) return fail(SMESH_ERR_INVALID, "NULL argument");
  const PropCall p = {weights, weights_memkind, mode, iterations, alpha, observed_threshold, out_mode, dont_care_threshold,
                      out_rows, out_labels, out_unreached, out_memkind};
  SMESH_TRY(check_prop_call(p));
  return smesh_aggregator_with_final_rows(ag, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    SMESH_TRY(check_rows_owner("face propagate", "face graph", ctx, gr->ctx, P, gr->F));
    return propagate_device_rows(gr, ctx, d_rows, C, p);
  });
}

int smesh_face_graph_normal_weights(const smesh_face_graph_t* gr, const int32_t* faces, const float* vertices, int vertices_memkind,
                                    uint32_t power, int two_sided, float* out_weights, int out_memkind) {
  if (!gr) return fail(SMESH_ERR_INVALID, "NULL face graph");
  if (power < 1 || power > SMESH_FG_MAX_POWER) return fail(SMESH_ERR_INVALID, "normal weights: power must lie in 1 .. 16");
  if (!memkind_ok(vertices_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "normal weights: bad memory kind");
  if ((gr->F && !faces) || (gr->F && !vertices) || (gr->nnz && !out_weights)) return fail(SMESH_ERR_INVALID, "normal weights: NULL argument");
  DeviceCtx* ctx = gr->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  if (gr->F == 0 || gr->nnz == 0) return SMESH_OK;
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  const int32_t* d_faces = nullptr;
  const float* d_vertices = nullptr;
  float4* nl = nullptr;
  uint32_t* bad = nullptr;
  Out<float> w;
  SMESH_TRY(on_device(ctx, tmp, faces, gr->F * 12, SMESH_MEM_HOST, &d_faces));
  SMESH_TRY(on_device(ctx, tmp, vertices, gr->V * 12, vertices_memkind, &d_vertices));
  SMESH_TRY(tmp.alloc(&nl, gr->F * 16));
  SMESH_TRY(tmp.alloc(&bad, 16));
  SMESH_TRY(w.init(tmp, out_weights, gr->nnz * 4, out_memkind));
  SMESH_HIP(hipMemsetAsync(bad, 0, 16, st));
  const dim3 gf((uint32_t)div_up(gr->F, kBlock)), b(kBlock);
  hipLaunchKernelGGL(k_fg_normals, gf, b, 0, st, d_faces, gr->F, gr->V, d_vertices, nl, bad);
  hipLaunchKernelGGL(k_fg_weights, gf, b, 0, st, (const uint32_t*)gr->offsets, (const uint32_t*)gr->neighbours, gr->F, (const float4*)nl,
                     power, two_sided, w.dev);
  SMESH_HIP(hipGetLastError());
  uint32_t h_bad = 0;
  SMESH_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
  SMESH_TRY(w.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (h_bad) return fail(SMESH_ERR_INVALID, "normal weights: a face index lies outside [0, " + std::to_string(gr->V) + ")");
  return SMESH_OK;
}

}  // extern "C"
