// fuse_rows.inc.hpp -- what k_fuse_tri_labels, k_fuse_tri_h16 and k_fuse_tri_sampled share (fusion_labels.hip, fusion_half.hip,
// fusion_sampled.hip): included INSIDE the anonymous namespace of those three translation units, after fuse_tri.inc.hpp, and by nobody
// else.  The three kernels have k_fuse_tri's structure -- lane = triangle, wave = 64 consecutive accumulator rows, tail blocks for
// the triangles over 8 x 8 pixels -- and differ in how a pixel's contribution is obtained.  Here, once each: the per-lane prologue
// (visible_masks), the tail waves' walk over the big-triangle queues (for_each_queued_triangle), Mesh.h:94-106 for one class vector
// (row_sum, add_pixel), the one-wave box fusion of class-vector kernels (fuse_box_rows), the way back of the dense-row LDS block
// (store_rows), the pieces of a partial chunk of 16-bit classes (load_part16), and the host side of a launch (check_fuse_rows,
// fuse_rows_grid, first_views, launch_fuse_rows).  What stays per kernel is a measured choice that the kernel's comment documents.
//
// The helpers are templates over the variant's own Args / View(s) structs, which agree on
//     View:  frags, idx, weights, big_queue, big_len, W, H          Args:  acc, F, C, iew, big_capacity, tri_blocks, big_blocks
// (no common base struct: the kernel-argument layouts stay what they were).

// Pieces of a row through pointer types that state the alignment there really is -- the element's -- which gfx950 global memory
// takes at any address.  Never past the row's end: the last pixel's row ends the allocation.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_a2 __attribute__((aligned(2)));
typedef u32x2 u32x2_a2 __attribute__((aligned(2)));
typedef uint32_t u32_a2 __attribute__((aligned(2)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));

// The first `r` = 1 .. 7 (wave-uniform) of eight 16-bit classes at `q`, packed two to a word, in pieces of 8, 4 and 2 bytes; the
// others come out as zero bits.
__device__ __forceinline__ u32x4 load_part16(const uint16_t* __restrict__ q, const int r) {
  u32x2 t8 = {0u, 0u};
  uint32_t t4 = 0u, t2 = 0u;
  if (r & 4) t8 = *reinterpret_cast<const u32x2_a2*>(q);
  if (r & 2) t4 = *reinterpret_cast<const u32_a2*>(q + (r & 4));
  if (r & 1) t2 = (uint32_t)q[r & 6];
  const uint32_t rest0 = (r & 2) ? t4 : t2, rest1 = (r & 2) ? t2 : 0u;   // what follows the 8-byte piece, if there is one
  u32x4 a;
  a.x = (r & 4) ? t8.x : rest0;
  a.y = (r & 4) ? t8.y : rest1;
  a.z = (r & 4) ? rest0 : 0u;
  a.w = (r & 4) ? rest1 : 0u;
  return a;
}

// The prologue of a main wave's lane, triangle `f`: per view the box origin (x0 | y0 << 16) and the mask of the triangle's VISIBLE
// pixels inside its <= 8 x 8 box; `big`: a box over 8 x 8 in some view -- the triangle is a tail wave's for all its views, and so is
// its row.  Returns the union of the masks (zero in every lane: nothing of these 64 triangles is visible).
// (k_fuse_tri_labels has the same lines written out in its kernel: as this helper they cost it SGPR spills and time, see there.)
template <int NV, typename Args, typename Views>
__device__ __forceinline__ unsigned long long visible_masks(const Args& a, const Views& vw, const uint64_t f, uint32_t (&org)[NV],
                                                            unsigned long long (&msk)[NV], bool& big) {
  big = false;
#pragma unroll
  for (int v = 0; v < NV; v++) { org[v] = 0u; msk[v] = 0ull; }
  if (f < a.F) {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const TriFrag rec = vw.v[v].frags[f];
      org[v] = (uint32_t)rec.x0 | ((uint32_t)rec.y0 << 16);
      msk[v] = rec.kind == 1 ? rec.mask : 0ull;
      big = big || rec.kind == 2;
    }
  }
  if (big) {
#pragma unroll
    for (int v = 0; v < NV; v++) msk[v] = 0ull;
  }
  // the masks of a view whose render says they need checking (fragment-queue overflow, direct rasteriser) are checked against that
  // view's index plane, which such a view always writes (k_fuse_tri's pass 1)
#pragma unroll
  for (int v = 0; v < NV; v++) {
    if (vw.v[v].big_len[1] == 0u) continue;
    const uint32_t* __restrict__ idx = vw.v[v].idx;
    unsigned long long m = msk[v], win = 0ull;
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      const uint64_t pix = (uint64_t)((org[v] & 0xFFFFu) + (uint32_t)(k >> 3)) * vw.v[v].H + (org[v] >> 16) + (uint32_t)(k & 7);
      if (idx[pix] == (uint32_t)f) win |= 1ull << k;
    }
    msk[v] = win;
  }
  unsigned long long any_win = 0ull;
#pragma unroll
  for (int v = 0; v < NV; v++) any_win |= msk[v];
  return any_win;
}

// Triangles with a box over 8 x 8 pixels in some view of the launch: one wave per queued triangle for ALL its views, first view first,
// so that no other wave touches its row (the main waves leave such triangles alone).  The walk over the concatenated queues is
// fuse_big_triangles': `chunk` entries per step, one per lane.  body(f, j, x0, y0, x1, y1) is called, wave-uniformly, once per view j
// in which triangle f has a non-empty clamped box: the record's box, or the 8 x 8 box of a view in which the triangle is small --
// which the body scans in THAT view's index plane, which is why the raster launch ahead of these kernels writes all planes as soon as
// one view has a queued triangle (raster.hip, kLabelsPlaneLevel).  UNROLL: NV copies of the body, else a loop over j (the view then
// comes from the kernel arguments by a wave-uniform index); which of the two is part of each kernel's measured register budget.
template <int NV, bool UNROLL, typename Args, typename Views, typename Body>
__device__ __forceinline__ void for_each_queued_triangle(const Args& a, const Views& vw, const uint32_t worker, const uint32_t nworkers, Body body) {
  uint32_t len[NV], total = 0u;
#pragma unroll
  for (int v = 0; v < NV; v++) { len[v] = min(*vw.v[v].big_len, a.big_capacity); total += len[v]; }
  const int l = threadIdx.x;
  const uint32_t chunk = max(1u, min((uint32_t)kWave, total / max(nworkers, 1u)));
  const uint32_t steps = (total + chunk - 1u) / chunk;
  for (uint32_t step = worker; step < steps; step += nworkers) {
    const uint32_t q = (uint32_t)l < chunk ? (uint32_t)l * steps + step : total;
    uint32_t fi = 0u;
    bool take = false;
    {
      uint32_t qq = q;
      bool located = q >= total;
      int jsel = -1;
#pragma unroll
      for (int j = 0; j < NV; j++) {
        if (!located) {
          if (qq < len[j]) { fi = vw.v[j].big_queue[qq]; jsel = j; located = true; }
          else qq -= len[j];
        }
      }
      if (jsel >= 0 && fi < a.F) {
        bool mine = false, earlier = false;
#pragma unroll
        for (int i = 0; i < NV; i++) {
          if (i <= jsel) {
            const bool counts = vw.v[i].frags[fi].kind == 2;
            if (i < jsel) earlier = earlier || counts;
            else mine = counts;
          }
        }
        take = mine && !earlier;   // a triangle queued by several views is taken from the queue of the first of them
      }
    }
    unsigned long long todo = __ballot(take);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)fi, src);   // wave-uniform; row = triangle (no re-ordered meshes here)
      auto visit = [&](const int j) __attribute__((always_inline)) {
        const TriFrag rec = vw.v[j].frags[f];
        if (rec.kind == 0) return;
        const int x0 = rec.x0, y0 = rec.y0;
        int x1, y1;
        if (rec.kind == 2) { x1 = (int)(rec.mask & 0xFFFFu); y1 = (int)((rec.mask >> 16) & 0xFFFFu); }
        else { x1 = x0 + 7; y1 = y0 + 7; }
        x1 = min(x1, (int)vw.v[j].W - 1); y1 = min(y1, (int)vw.v[j].H - 1);
        if (x1 < x0 || y1 < y0) return;
        body(f, j, x0, y0, x1, y1);
      };
      if constexpr (UNROLL) {
#pragma unroll
        for (int j = 0; j < NV; j++) visit(j);
      } else {
#pragma nounroll
        for (int j = 0; j < NV; j++) visit(j);
      }
    }
  }
}

// Mesh.h:94-106 for one pixel's class vector `p` with weight `w` into `dst` (a row in registers, or a tail wave's partial sums).
template <int CT, int KIND>
__device__ __forceinline__ void add_pixel(const float (&p)[CT], int C, float w, float (&dst)[CT]) {
  if (KIND == SMESH_AGG_SUMMAX) {
    int am = 0;
    float best = p[0];   // (not p[am]: a run-time register index would go through scratch)
#pragma unroll
    for (int c = 1; c < CT; c++) if (c < C) if (p[c] > best) { best = p[c]; am = c; }
#pragma unroll
    for (int c = 0; c < CT; c++) if (c < C) if (c == am) dst[c] = dst[c] + p[c] * w;
  } else {
#pragma unroll
    for (int c = 0; c < CT; c++) if (c < C) dst[c] = dst[c] + p[c] * w;
  }
}

template <int CT>
__device__ __forceinline__ float row_sum(const float (&p)[CT], int C) {
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < CT; c++) if (c < C) sum = sum + p[c];   // tt::sum, sequential float32
  return sum;
}

// One queued triangle `f` in one view of class vectors: one WAVE, lanes over the pixels of the box [x0, x1] x [y0, y1] of the view's
// index plane, load_row(x, y, p) gives a visible pixel's class vector in CT float32 registers, per-lane partial sums combined by a
// butterfly; lane c then adds class c to the row, which nobody else touches in this launch.  A tree order: the 1e-5 path, like fuse_box.
template <int CT, int KIND, typename Args, typename View, typename LoadRow>
__device__ __forceinline__ void fuse_box_rows(const Args& a, const View& vw, const uint32_t f, const int x0, const int y0, const int x1, const int y1,
                                              LoadRow load_row) {
  const int C = (int)a.C;
  const int l = threadIdx.x;
  const uint32_t bh = (uint32_t)(y1 - y0 + 1);
  const uint32_t npx = (uint32_t)(x1 - x0 + 1) * bh;   // (W, H <= 65536 and W * H < 2^29: fits)
  const uint32_t* __restrict__ idx = vw.idx;
  uint32_t cnt = 0;
  for (uint32_t i = l; i < npx; i += kWave) cnt += idx[(uint64_t)((uint32_t)x0 + i / bh) * vw.H + ((uint32_t)y0 + i % bh)] == f ? 1u : 0u;
  const uint32_t n = wave_sum_u(cnt);
  if (n == 0) return;
  const float w0 = a.iew * (1.0f / (float)n) + (1 - a.iew) * 1.0f;
  float part[CT];
#pragma unroll
  for (int c = 0; c < CT; c++) part[c] = 0.0f;
  for (uint32_t i = l; i < npx; i += kWave) {
    const uint32_t x = (uint32_t)x0 + i / bh, y = (uint32_t)y0 + i % bh;
    const uint64_t pix = (uint64_t)x * vw.H + y;
    if (idx[pix] != f) continue;
    float p[CT];
    load_row(x, y, p);
    if (!(row_sum<CT>(p, C) > 0.5f)) continue;                                  // Mesh.h:98
    const float w = w0 * (vw.weights ? vw.weights[pix] : 1.0f);                 // :103
    add_pixel<CT, KIND>(p, C, w, part);
  }
  float mine = 0.0f;
#pragma unroll
  for (int c = 0; c < CT; c++) if (c < C) {
    const float v = wave_sum(part[c]);
    if (l == c) mine = v;
  }
  if (l < C) {
    float* __restrict__ row = a.acc + (uint64_t)f * C;
    row[l] = row[l] + mine;
  }
}

// ---- the wave's 64 accumulator rows in LDS, dense: row r at srow[r * C] (k_fuse_tri_h16, k_fuse_tri_sampled) ---------------------
// (k_fuse_tri_labels keeps its own, strided block: its pixels are read-modify-writes at srow[row * stride + label], which at a dense
// even C would put the 64 lanes on few banks, so its rows are C | 1 floats apart and every float4 of the block is taken apart on the
// way in and out -- a different loop, not a parameter of this one.)
constexpr int rows_quads(int ct) { return (kWave * ct / 4 + kWave - 1) / kWave; }   // float4 per lane of a 64-row block of ct-float rows

// The rows back to the accumulator: row `f` of this lane from `accr`, the block of the wave at `blk`.
template <int CT>
__device__ __forceinline__ void store_rows(float* acc, float* srow, float* blk, const uint64_t f, const int nrows,
                                           const int C, const bool big, const bool any_win, const float (&accr)[CT]) {
  const int l = threadIdx.x;
  // each lane parks its row ...
#pragma unroll
  for (int c = 0; c < CT; c++) if (c < C) srow[l * C + c] = accr[c];
  wave_sync();
  if (nrows != kWave || __ballot(big) != 0ull) {
    // some of these 64 rows belong to queued triangles, which the tail waves of this launch update meanwhile (or the block is the
    // mesh's last, partial one): every lane that added something stores its own row
    if (any_win) {
      float* __restrict__ row = acc + f * C;
      const float* __restrict__ mine = srow + l * C;
      for (int c = 0; c < C; c++) row[c] = mine[c];
    }
    return;
  }
  // ... and the block goes back as it came
  f4* b4 = reinterpret_cast<f4*>(blk);
  const f4* s4 = reinterpret_cast<const f4*>(srow);
  for (int q = l; q < kWave * C / 4; q += kWave) b4[q] = s4[q];
}

// ---- the host side of a launch --------------------------------------------------------------------------------------------------
// What the three smesh_*_fuse_triangles check alike and fill in alike.  `who`: "fuse_triangles_half" ...; `call`: the entry point
// named to a caller whose accumulator is reduce-scattered; `max_classes` 0: any class count (the label kernel).
template <typename Args>
int check_fuse_rows(const char* who, const char* call, smesh_aggregator* a, uint64_t F, int nviews, uint32_t max_classes, Args* t, int* kind) {
  const std::string p = std::string(who) + ": ";
  SMESH_TRY(smesh_aggregator_refuse_scattered(a, call));
  if (nviews != 1 && nviews != 2 && nviews != 4 && nviews != 8) return fail(SMESH_ERR_INVALID, p + "unsupported view count");
  uint64_t P;
  smesh_aggregator_label_target(a, &t->acc, &P, &t->C, kind, &t->iew);
  if (!max_classes) {
    if (*kind == SMESH_AGG_MUL || P != F) return fail(SMESH_ERR_INVALID, p + "Sum / Summax over the renderer's triangles only");
  } else if (*kind == SMESH_AGG_MUL || P != F || t->C == 0 || t->C > max_classes) {
    return fail(SMESH_ERR_INVALID, p + "Sum / Summax over the renderer's triangles, at most " + std::to_string(max_classes) + " classes");
  }
  return SMESH_OK;
}

// The grid of a launch: one block per 64 triangles, then the tail blocks -- none where every view is PROVEN free of triangles over
// 8 x 8 pixels (RenderedView::no_big).
template <typename Args>
dim3 fuse_rows_grid(DeviceCtx* ctx, uint64_t F, uint32_t big_capacity, const RenderedView* views, int nviews, Args* t) {
  bool no_big = true;
  for (int v = 0; v < nviews; v++) no_big = no_big && views[v].no_big;
  t->F = F;
  t->big_capacity = big_capacity;
  t->tri_blocks = (uint32_t)div_up(F, kWave);
  t->big_blocks = no_big ? 0u : 16u * (uint32_t)std::max(1, ctx->num_cus);
  smesh_note_fuse_rows_views(ctx, views, nviews);   // (reporting only: the read-only option "last_fuse_flagged_views")
  return dim3(t->tri_blocks + t->big_blocks);
}

// The first NV of eight views as the kernel argument of an NV-view instance.
template <template <int> class Views, int NV>
Views<NV> first_views(const Views<8>& tv) {
  Views<NV> w;
  for (int v = 0; v < NV; v++) w.v[v] = tv.v[v];
  return w;
}

// launch(ct, kind, nv) with the run-time class slots `ct` (8, 16 .. 48; 0: the kernel has none and one kind), aggregator kind (Sum /
// Summax) and view count (1, 2, 4, 8) as std::integral_constant arguments; then the instance goes on record (reporting only: the
// read-only options "last_fuse_slot" / "last_fuse_views").
template <bool SLOTS, typename Launch>
void launch_fuse_rows(int ct, int kind, int nviews, Launch launch) {
  auto by_views = [&](auto CT, auto KIND) {
    switch (nviews) {
      case 1: launch(CT, KIND, std::integral_constant<int, 1>()); break;
      case 2: launch(CT, KIND, std::integral_constant<int, 2>()); break;
      case 4: launch(CT, KIND, std::integral_constant<int, 4>()); break;
      default: launch(CT, KIND, std::integral_constant<int, 8>()); break;
    }
  };
  auto by_kind = [&](auto CT) {
    if (SLOTS && kind == SMESH_AGG_SUMMAX) by_views(CT, std::integral_constant<int, SMESH_AGG_SUMMAX>());
    else by_views(CT, std::integral_constant<int, SMESH_AGG_SUM>());
  };
  if constexpr (SLOTS) {
    switch (ct) {
      case 8:  by_kind(std::integral_constant<int, 8>()); break;
      case 16: by_kind(std::integral_constant<int, 16>()); break;
      case 24: by_kind(std::integral_constant<int, 24>()); break;
      case 32: by_kind(std::integral_constant<int, 32>()); break;
      case 40: by_kind(std::integral_constant<int, 40>()); break;
      default: by_kind(std::integral_constant<int, 48>()); break;
    }
  } else {
    by_kind(std::integral_constant<int, 0>());
  }
  smesh_set_last_fuse_instance(ct, nviews);
}
