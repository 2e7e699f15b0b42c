// points.hip -- fused results for points that are not the mesh's vertices (include/smesh_points.h): a uniform grid over the faces of a
// mesh, built on the device, the closest face of every query point, and the gather of the fused rows of those faces.
//
// Reference: eval-scannet/eval_scannet.py:245 has per-vertex metrics only where the fused mesh is the ground-truth mesh; nothing there
// maps the ground truth's vertices onto another mesh's faces.
//
// The closest face is defined to the bit (smesh_points.h) as the result of the exhaustive scan: faces are compared by (dist2, f), so
// neither the order in which the grid walk meets them nor meeting one twice can change the result.  What the walk has to get right is
// WHEN TO STOP: k_pts_nearest_grid, "the bound".
#include "mesh_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/smesh_points.h"

using namespace smesh;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kMaxDim = 256;            // cells per axis, at most
constexpr int kEdgeStride = kMaxDim + 1;
// A face whose box overlaps more cells than this is kept out of the cells' lists and tested by every query instead (one ground plane
// must not fill the grid).  Not tuned: the issue's starting value.  A small mesh never has that many cells, so the same holds for a
// face whose box overlaps more than an eighth of the grid and more than kLargeFloor cells: most queries would meet it anyway.
constexpr uint32_t kLargeCells = 4096;
constexpr uint32_t kLargeFloor = 64;
// (twice the area)^2 over (longest edge)^4 -- the square of height over longest edge, roughly -- below which a face counts as without
// area and joins the same list: the rule's case 7 divides by a sum of cancelling products there, and its r need not lie on the face,
// which is the one assumption the bound below makes.
constexpr float kSliver = 1e-8f;

#include "scan.inc.hpp"   // k_scan_tiles, k_scan_sums, k_scan_add

struct Grid {
  float lo[3];               // lower corner of the bounding box of the finite vertices
  float inv[3];              // cells per unit length (0: the axis has no extent and one cell)
  float size[3];             // nominal edge length of a cell
  int dims[3];
  float maxabs;              // largest |coordinate| of a finite vertex
  const float* edges;        // [2][3][kEdgeStride] cell borders as cell_of sees them (k_pts_edges)
  const uint32_t* cell_start;   // [cells + 1]
  const uint32_t* cell_list;    // [entries] faces of cell c: cell_list[cell_start[c] .. cell_start[c + 1]), any order
  const uint32_t* large;        // [nlarge] faces every query tests
  uint32_t nlarge;
  const float4* tris;        // [F][3] the vertices a, b, c of every face (w unused)
};

// The cell of a coordinate along one axis.  MONOTONE in x: a rounded subtraction, a rounded product with a non-negative number, floor
// and the clamps all are.  The whole index rests on this and on nothing else about the function.
__device__ __forceinline__ int cell_of(float x, float lo, float inv, int n) {
  const float t = floorf((x - lo) * inv);
  return (int)fminf(fmaxf(t, 0.0f), (float)(n - 1));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- building the index --------------------------------------------------------------------------------------------------------
// floats as unsigned integers of the same order
__device__ __forceinline__ uint32_t ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// box[0..2]: smallest x, y, z, box[3..5]: largest, as `ordered` values; starts at (0xFFFFFFFF x 3, 0 x 3)
__global__ __launch_bounds__(kBlock) void k_pts_bbox(const float* __restrict__ vertices, uint64_t V, uint32_t* __restrict__ box) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  if (v < V) {
    const float x = vertices[v * 3], y = vertices[v * 3 + 1], z = vertices[v * 3 + 2];
    if (finite3(x, y, z)) {
      mn[0] = mx[0] = ordered(x);
      mn[1] = mx[1] = ordered(y);
      mn[2] = mx[2] = ordered(z);
    }
  }
  for (int d = kWave >> 1; d > 0; d >>= 1)
    for (int k = 0; k < 3; k++) {
      mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], d, kWave));
      mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], d, kWave));
    }
  if ((threadIdx.x & (kWave - 1)) == 0)
    for (int k = 0; k < 3; k++) {
      if (mn[k] != 0xFFFFFFFFu) atomicMin(&box[k], mn[k]);
      if (mx[k] != 0u) atomicMax(&box[3 + k], mx[k]);
    }
}

__global__ __launch_bounds__(kBlock) void k_pts_pack(const float* __restrict__ vertices, uint64_t V, const int32_t* __restrict__ faces, uint64_t F,
                                                     float4* __restrict__ tris, uint32_t* __restrict__ bad) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  for (int k = 0; k < 3; k++) {
    const int v = faces[f * 3 + k];
    float4 p = make_float4(NAN, NAN, NAN, 0.0f);
    if (v < 0 || (uint64_t)v >= V) atomicOr(bad, 1u);
    else p = make_float4(vertices[(uint64_t)v * 3], vertices[(uint64_t)v * 3 + 1], vertices[(uint64_t)v * 3 + 2], 0.0f);
    tris[f * 3 + k] = p;
  }
}

// The cell borders along each axis AS cell_of SEES THEM.  For 0 < i < n:
//   up[i]   (edges[axis][i])      a float with cell_of(up[i]) >= i, so that cell_of(x) <  i implies x < up[i]
//   down[i] (edges[3 + axis][i])  a float with cell_of(down[i]) < i, so that cell_of(x) >= i implies x > down[i]
// (both by monotonicity), found by stepping from lo + i * size float by float.  A border that is not found within the steps allowed
// is left at +inf / -inf: every bound that uses it comes out as 0, which is conservative.
__global__ __launch_bounds__(kBlock) void k_pts_edges(Grid g, float* __restrict__ edges) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 3 * kEdgeStride) return;
  const int axis = t / kEdgeStride, i = t % kEdgeStride, n = g.dims[axis];
  float up = INFINITY, down = -INFINITY;
  if (i > 0 && i < n) {
    const float lo = g.lo[axis], inv = g.inv[axis];
    float e = lo + (float)i * g.size[axis];
    if (cell_of(e, lo, inv, n) >= i) {
      up = e;
      for (int k = 0; k < 256; k++) {
        e = nextafterf(e, -INFINITY);
        if (cell_of(e, lo, inv, n) < i) { down = e; break; }
        up = e;
      }
    } else {
      down = e;
      for (int k = 0; k < 256; k++) {
        e = nextafterf(e, INFINITY);
        if (cell_of(e, lo, inv, n) >= i) { up = e; break; }
        down = e;
      }
    }
  }
  edges[axis * kEdgeStride + i] = up;
  edges[(3 + axis) * kEdgeStride + i] = down;
}

// Where a face goes: 1 the list every query tests, 2 the cells lo[] .. hi[] of its bounding box.  A face with a non-finite vertex has
// no box; with a NaN it can never win, but with an infinite vertex the rule's cases 1, 2 and 4 can still answer from a finite one,
// and the result is the exhaustive scan's: such faces are tested by every query.
__device__ __forceinline__ int face_cells(const Grid& g, uint64_t f, int lo[3], int hi[3]) {
  const float4 a = g.tris[f * 3], b = g.tris[f * 3 + 1], c = g.tris[f * 3 + 2];
  if (!finite3(a.x, a.y, a.z) || !finite3(b.x, b.y, b.z) || !finite3(c.x, c.y, c.z)) return 1;
  const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float wx = c.x - b.x, wy = c.y - b.y, wz = c.z - b.z;
  const float nn = (nx * nx + ny * ny) + nz * nz;
  const float longest = fmaxf(fmaxf((ux * ux + uy * uy) + uz * uz, (vx * vx + vy * vy) + vz * vz), (wx * wx + wy * wy) + wz * wz);
  if (!(nn > kSliver * (longest * longest))) return 1;
  const float mn[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
  const float mx[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
  uint64_t cells = 1;
  for (int k = 0; k < 3; k++) {
    lo[k] = cell_of(mn[k], g.lo[k], g.inv[k], g.dims[k]);
    hi[k] = cell_of(mx[k], g.lo[k], g.inv[k], g.dims[k]);
    cells *= (uint64_t)(hi[k] - lo[k] + 1);
  }
  const uint64_t grid = (uint64_t)g.dims[0] * g.dims[1] * g.dims[2];
  return cells > kLargeCells || (cells > kLargeFloor && cells * 8 > grid) ? 1 : 2;
}

// counters: [0] faces in the `large` list, [1] fill cursor of that list, [2..3] entries of the cells' lists as one uint64
__global__ __launch_bounds__(kBlock) void k_pts_count(Grid g, uint64_t F, uint32_t* __restrict__ count, uint32_t* __restrict__ counters) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long mine = 0;
  if (f < F) {
    int lo[3], hi[3];
    const int kind = face_cells(g, f, lo, hi);
    if (kind == 1) atomicAdd(&counters[0], 1u);
    if (kind == 2)
      for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++)
          for (int x = lo[0]; x <= hi[0]; x++, mine++) atomicAdd(&count[((uint64_t)z * g.dims[1] + y) * g.dims[0] + x], 1u);
  }
  for (int d = kWave >> 1; d > 0; d >>= 1) mine += __shfl_xor(mine, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(reinterpret_cast<unsigned long long*>(counters + 2), mine);
}

// `cursor` is all zero; the order of a cell's faces is whatever the atomics make it, and no result depends on it.
__global__ __launch_bounds__(kBlock) void k_pts_fill(Grid g, uint64_t F, uint32_t* __restrict__ cursor, uint32_t* __restrict__ cell_list,
                                                     uint32_t* __restrict__ large, uint32_t* __restrict__ counters) {
  const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int lo[3], hi[3];
  const int kind = face_cells(g, f, lo, hi);
  if (kind == 1) large[atomicAdd(&counters[1], 1u)] = (uint32_t)f;
  if (kind == 2)
    for (int z = lo[2]; z <= hi[2]; z++)
      for (int y = lo[1]; y <= hi[1]; y++)
        for (int x = lo[0]; x <= hi[0]; x++) {
          const uint64_t cell = ((uint64_t)z * g.dims[1] + y) * g.dims[0] + x;
          cell_list[g.cell_start[cell] + atomicAdd(&cursor[cell], 1u)] = (uint32_t)f;
        }
}

// ---- the rule ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot3(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }

// dist2(q, f) of smesh_points.h, operation by operation (the file is compiled with -ffp-contract=off; `/` is hipcc's correctly
// rounded division).
__device__ __forceinline__ float dist2_face(float qx, float qy, float qz, const float4 a, const float4 b, const float4 c) {
  const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
  const float acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
  const float apx = qx - a.x, apy = qy - a.y, apz = qz - a.z;
  const float bpx = qx - b.x, bpy = qy - b.y, bpz = qz - b.z;
  const float cpx = qx - c.x, cpy = qy - c.y, cpz = qz - c.z;
  const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  float rx, ry, rz;
  if (d1 <= 0.0f && d2 <= 0.0f) {
    rx = a.x; ry = a.y; rz = a.z;
  } else if (d3 >= 0.0f && d4 <= d3) {
    rx = b.x; ry = b.y; rz = b.z;
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    const float t = d1 / (d1 - d3);
    rx = a.x + t * abx; ry = a.y + t * aby; rz = a.z + t * abz;
  } else if (d6 >= 0.0f && d5 <= d6) {
    rx = c.x; ry = c.y; rz = c.z;
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    const float t = d2 / (d2 - d6);
    rx = a.x + t * acx; ry = a.y + t * acy; rz = a.z + t * acz;
  } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    const float t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    rx = b.x + t * (c.x - b.x); ry = b.y + t * (c.y - b.y); rz = b.z + t * (c.z - b.z);
  } else {
    const float den = 1.0f / ((va + vb) + vc);
    const float v = vb * den, w = vc * den;
    rx = (a.x + abx * v) + acx * w; ry = (a.y + aby * v) + acy * w; rz = (a.z + abz * v) + acz * w;
  }
  const float ex = qx - rx, ey = qy - ry, ez = qz - rz;
  return dot3(ex, ey, ez, ex, ey, ez);
}

struct Best {
  float d2;
  int f;
};

__device__ __forceinline__ void test_face(const float4* __restrict__ tris, uint32_t f, float qx, float qy, float qz, Best& best) {
  const float d = dist2_face(qx, qy, qz, tris[(uint64_t)f * 3], tris[(uint64_t)f * 3 + 1], tris[(uint64_t)f * 3 + 2]);
  if (d < best.d2 || (d == best.d2 && (int)f < best.f)) { best.d2 = d; best.f = (int)f; }   // (NaN and +inf: neither holds)
}

__device__ __forceinline__ void write_result(const Best& best, float r2, uint64_t p, int32_t* out_face, float* out_dist2) {
  const bool in = best.f >= 0 && best.d2 <= r2;
  out_face[p] = in ? best.f : -1;
  if (out_dist2) out_dist2[p] = in ? best.d2 : INFINITY;
}

// The exhaustive scan: one lane per point over all F faces (option "points_grid" 0: a test hook and the bench's baseline).
__global__ __launch_bounds__(kBlock) void k_pts_nearest_all(const float* __restrict__ points, uint64_t N, const float4* __restrict__ tris, uint64_t F,
                                                            float r2, int32_t* __restrict__ out_face, float* __restrict__ out_dist2) {
  const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= N) return;
  const float qx = points[p * 3], qy = points[p * 3 + 1], qz = points[p * 3 + 2];
  Best best = {INFINITY, -1};
  if (finite3(qx, qy, qz))
    for (uint64_t f = 0; f < F; f++) test_face(tris, (uint32_t)f, qx, qy, qz, best);
  write_result(best, r2, p, out_face, out_dist2);
}

// x rounded towards zero by one float, 0 for anything that is not positive: what turns a float that is within half a unit in the last
// place of a real lower bound into a lower bound.
__device__ __forceinline__ float shrink(float x) { return x > 0.0f ? __uint_as_float(__float_as_uint(x) - 1u) : 0.0f; }

// One lane per point, the points in the order of their cells (perm), so that the lanes of a wave walk neighbouring cells.  A lane
// tests the `large` list, then the cells of the Chebyshev shells s = 0, 1, 2, ... around its own (clamped) cell, and stops after a
// shell when its best cannot be beaten from outside the box of cells it has explored.
//
// THE BOUND.  face_cells lists a face in every cell of its bounding box, cell by cell_of; cell_of is monotone, so for every point p ON
// a listed face the face is in the list of the cell (cell_of(p.x), cell_of(p.y), cell_of(p.z)).  After shell s the lane has seen all
// faces of the cells a0 .. a1 (per axis).  A point p of a face it has NOT seen therefore has, on some axis, cell_of(p) < a0 -- then
// p < up[a0] (k_pts_edges) -- or cell_of(p) > a1 -- then p > down[a1 + 1].  So |q - p| >= m, the smallest of q - up[a0] and
// down[a1 + 1] - q over the axes and sides that are not at the grid's edge yet; cells 0 and n - 1 reach to infinity (the clamps), so a
// side at the grid's edge hides nothing, and a query point outside the grid needs no special case.  Each difference is rounded DOWN
// (shrink; a negative one counts as 0).  The rule's own r is a point of the face up to rounding (a convex combination of a, b, c in
// every case; faces where cancellation could throw case 7's r off the face are in the `large` list): its float32 dist2 is at least
// (|q - p| - delta)^2 (1 - 2^-21) with delta = 2^-19 times the largest |coordinate| involved (some 32 units in the last place of that
// coordinate, against about a dozen roundings in r and e).  The lane stops when best <= b, that value rounded down once more.
__global__ __launch_bounds__(kBlock) void k_pts_nearest_grid(const float* __restrict__ points, const uint32_t* __restrict__ perm, uint64_t N, Grid g,
                                                             float r2, int32_t* __restrict__ out_face, float* __restrict__ out_dist2) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const uint64_t p = perm[i];
  const float q[3] = {points[p * 3], points[p * 3 + 1], points[p * 3 + 2]};
  Best best = {INFINITY, -1};
  if (finite3(q[0], q[1], q[2])) {
    for (uint32_t k = 0; k < g.nlarge; k++) test_face(g.tris, g.large[k], q[0], q[1], q[2], best);
    int c[3];
    for (int k = 0; k < 3; k++) c[k] = cell_of(q[k], g.lo[k], g.inv[k], g.dims[k]);
    const float delta = 0x1p-19f * fmaxf(fmaxf(g.maxabs, fabsf(q[0])), fmaxf(fabsf(q[1]), fabsf(q[2])));
    const int nx = g.dims[0], ny = g.dims[1];
    for (int s = 0;; s++) {
      int a0[3], a1[3];
      for (int k = 0; k < 3; k++) { a0[k] = max(c[k] - s, 0); a1[k] = min(c[k] + s, g.dims[k] - 1); }
      for (int z = a0[2]; z <= a1[2]; z++)
        for (int y = a0[1]; y <= a1[1]; y++) {
          const uint64_t row = ((uint64_t)z * ny + y) * nx;
          if (abs(z - c[2]) == s || abs(y - c[1]) == s) {     // a row of the shell's faces: its cells' lists are one run
            const uint32_t end = g.cell_start[row + a1[0] + 1];
            for (uint32_t k = g.cell_start[row + a0[0]]; k < end; k++) test_face(g.tris, g.cell_list[k], q[0], q[1], q[2], best);
          } else {                                            // the two cells where the row pierces the shell
            for (int side = 0; side < 2; side++) {
              const int x = side ? c[0] + s : c[0] - s;
              if (x < 0 || x >= nx) continue;
              const uint32_t end = g.cell_start[row + x + 1];
              for (uint32_t k = g.cell_start[row + x]; k < end; k++) test_face(g.tris, g.cell_list[k], q[0], q[1], q[2], best);
            }
          }
        }
      bool all = true;
      float m = INFINITY;
      for (int k = 0; k < 3; k++) {
        if (a0[k] > 0) { all = false; m = fminf(m, shrink(q[k] - g.edges[k * kEdgeStride + a0[k]])); }
        if (a1[k] < g.dims[k] - 1) { all = false; m = fminf(m, shrink(g.edges[(3 + k) * kEdgeStride + a1[k] + 1] - q[k])); }
      }
      if (all) break;                                         // the box is the whole grid
      m = shrink(m - delta);
      float b = m * m;
      b = shrink(b - b * 0x1p-20f);
      // nothing outside can win, or be within max_distance.  (b > 0: the margins then put b strictly below every unseen dist2; at
      // b == 0 an unseen face could still tie with a best of 0 and win by its lower index.)
      if (b > 0.0f && (best.d2 <= b || b > r2)) break;
    }
  }
  write_result(best, r2, p, out_face, out_dist2);
}

// ---- binning the query points --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_pts_cells(const float* __restrict__ points, uint64_t N, Grid g, uint32_t* __restrict__ cell,
                                                      uint32_t* __restrict__ count) {
  const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= N) return;
  const float x = points[p * 3], y = points[p * 3 + 1], z = points[p * 3 + 2];
  uint32_t c = 0;      // (a non-finite point: any cell, it walks none)
  if (finite3(x, y, z))
    c = (uint32_t)(((uint64_t)cell_of(z, g.lo[2], g.inv[2], g.dims[2]) * g.dims[1] + cell_of(y, g.lo[1], g.inv[1], g.dims[1])) * g.dims[0] +
                   cell_of(x, g.lo[0], g.inv[0], g.dims[0]));
  cell[p] = c;
  atomicAdd(&count[c], 1u);
}

__global__ __launch_bounds__(kBlock) void k_pts_perm(const uint32_t* __restrict__ cell, uint64_t N, const uint32_t* __restrict__ start,
                                                     uint32_t* __restrict__ cursor, uint32_t* __restrict__ perm) {
  const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= N) return;
  const uint32_t c = cell[p];
  perm[start[c] + atomicAdd(&cursor[c], 1u)] = (uint32_t)p;
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------
struct PointGatherArgs {
  const float* rows;       // [F, C]
  const int32_t* faces;    // [N]
  uint64_t F, N;
  uint32_t C;
  int mode;
  float threshold;
  float* out_rows;         // [N, C] or null
  int32_t* out_labels;     // [N] or null
  uint32_t* bad;           // set when a face >= F is met
};

// A group of G lanes owns one point; lane l of the group owns the classes l, l + G, ...  The row total is added in ascending class
// order by every lane of the group (one cross-lane read per class), as k_vertex_gather does it, so all of them hold it for the division.
template <int G>
__global__ __launch_bounds__(kBlock) void k_point_gather(PointGatherArgs a) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t item = tid / G;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int gl = lane & (G - 1), gbase = lane - gl;
  const bool valid = item < a.N;          // (a whole group at a time: nobody leaves before the cross-lane steps)
  const uint32_t C = a.C;
  int64_t f = valid ? (int64_t)a.faces[item] : -1;
  if (f >= (int64_t)a.F) {
    if (gl == 0) atomicOr(a.bad, 1u);
    f = -1;
  }
  const bool has = f >= 0;
  const float* const row = a.rows + (has ? (uint64_t)f * C : 0);
  float total = 0.0f, best = 0.0f;
  int best_c = 0x7FFFFFFF;
  if (a.out_labels != nullptr || a.mode != SMESH_VTX_SUMS) {
    for (uint32_t c0 = 0; c0 < C; c0 += G) {
      const uint32_t c = c0 + gl;
      const float x = has && c < C ? row[c] : 0.0f;
      const int width = (int)min((uint32_t)G, C - c0);
      if (G == 1) total += x;
      else
        for (int l = 0; l < width; l++) total += __shfl(x, gbase + l, kWave);
      if (c < C && (best_c == 0x7FFFFFFF || x > best)) { best = x; best_c = (int)c; }
    }
  }
  const bool dont_care = !has || total < a.threshold;
  if (a.out_labels) {
#pragma unroll
    for (int d = G >> 1; d > 0; d >>= 1) {
      const float ob = __shfl_xor(best, d, kWave);
      const int oc = __shfl_xor(best_c, d, kWave);
      if (oc != 0x7FFFFFFF && (best_c == 0x7FFFFFFF || ob > best || (ob == best && oc < best_c))) { best = ob; best_c = oc; }
    }
    if (valid && gl == 0) a.out_labels[item] = dont_care ? -1 : best_c;
  }
  if (a.out_rows && valid)
    for (uint32_t c = gl; c < C; c += G) {
      const float x = has ? row[c] : 0.0f;
      a.out_rows[item * C + c] = a.mode == SMESH_VTX_SUMS ? x : dont_care ? 0.0f : x / total;
    }
}

template <int G>
void launch_point_gather(const PointGatherArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_point_gather<G>), dim3((uint32_t)div_up(a.N * G, kBlock)), dim3(kBlock), 0, st, a);
}

int check_point_gather_args(uint32_t C, uint64_t N, const void* faces, int faces_memkind, int mode, const void* out_rows,
                            const void* out_labels, int out_memkind) {
  SMESH_TRY(check_gather_args("point gather", C, mode, out_rows, out_labels, faces_memkind, out_memkind));
  if (N && !faces) return fail(SMESH_ERR_INVALID, "point gather: NULL faces");
  if (N >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "point gather: N must stay below 2^32");
  return SMESH_OK;
}

// The gather over rows that are on the device already.  Context locked, device current.
int gather_device_rows(DeviceCtx* ctx, const float* d_rows, uint64_t F, uint32_t C, const int32_t* faces, uint64_t N, int faces_memkind, int mode,
                       float threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  if (N == 0) return SMESH_OK;
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  PointGatherArgs a = {};
  a.rows = d_rows;
  a.F = F;
  a.N = N;
  a.C = C;
  a.mode = mode;
  a.threshold = threshold;
  SMESH_TRY(on_device(ctx, tmp, faces, N * 4, faces_memkind, &a.faces));
  SMESH_TRY(tmp.alloc(&a.bad, 16));
  SMESH_HIP(hipMemsetAsync(a.bad, 0, 16, st));
  Out<float> rows;
  Out<int32_t> labels;
  SMESH_TRY(rows.init(tmp, out_rows, (size_t)N * C * 4, out_memkind));
  SMESH_TRY(labels.init(tmp, out_labels, (size_t)N * 4, out_memkind));
  a.out_rows = rows.dev;
  a.out_labels = labels.dev;
  if (C <= 1) launch_point_gather<1>(a, st);
  else if (C <= 2) launch_point_gather<2>(a, st);
  else if (C <= 4) launch_point_gather<4>(a, st);
  else if (C <= 8) launch_point_gather<8>(a, st);
  else if (C <= 16) launch_point_gather<16>(a, st);
  else if (C <= 32) launch_point_gather<32>(a, st);
  else launch_point_gather<kWave>(a, st);
  SMESH_HIP(hipGetLastError());
  uint32_t h_bad = 0;
  SMESH_HIP(hipMemcpyAsync(&h_bad, a.bad, 4, hipMemcpyDeviceToHost, st));
  SMESH_TRY(rows.copy_back(st));
  SMESH_TRY(labels.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  if (h_bad) return fail(SMESH_ERR_INVALID, "point gather: a face index is not below " + std::to_string(F));
  return SMESH_OK;
}

float unordered(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

}  // namespace

struct smesh_surface_index {
  DeviceCtx* ctx = nullptr;
  uint64_t F = 0, entries = 0, cells = 1;
  Grid grid = {};
  float4* tris = nullptr;
  float* edges = nullptr;
  uint32_t* cell_start = nullptr;
  uint32_t* cell_list = nullptr;
  uint32_t* large = nullptr;
};

namespace {

// The grid's shape from the bounding box: about one cell per face (cells of equal edge length over the axes that have an extent),
// every dimension in [1, kMaxDim].
void shape_grid(Grid& g, const float lo[3], const float hi[3], bool any, uint64_t F) {
  double ext[3], vol = 1.0;
  int axes = 0;
  for (int k = 0; k < 3; k++) {
    ext[k] = any ? (double)hi[k] - (double)lo[k] : 0.0;
    if (ext[k] > 0.0) { vol *= ext[k]; axes++; }
  }
  const double edge = axes ? std::pow(vol / (double)std::max<uint64_t>(F, 1), 1.0 / axes) : 0.0;
  g.maxabs = 0.0f;
  for (int k = 0; k < 3; k++) {
    int n = 1;
    if (ext[k] > 0.0 && edge > 0.0) n = (int)std::min<double>(kMaxDim, std::max(1.0, std::ceil(ext[k] / edge)));
    const float extent = any ? hi[k] - lo[k] : 0.0f;      // (float32, as the kernels see the box)
    if (!(extent > 0.0f) || !std::isfinite(extent)) n = 1;
    g.dims[k] = n;
    g.lo[k] = any ? lo[k] : 0.0f;
    g.size[k] = n > 1 ? extent / (float)n : 0.0f;
    g.inv[k] = n > 1 ? (float)n / extent : 0.0f;
    if (!std::isfinite(g.inv[k]) || !(g.size[k] > 0.0f)) { g.dims[k] = 1; g.inv[k] = 0.0f; g.size[k] = 0.0f; }
    if (any) g.maxabs = std::max(g.maxabs, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
  }
}

int build_index(smesh_surface_index* s, const float* vertices, uint64_t V, const int32_t* faces) {
  DeviceCtx* ctx = s->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t F = s->F;
  TempBlocks tmp;
  float* d_vertices = nullptr;
  int32_t* d_faces = nullptr;
  uint32_t *box = nullptr, *counters = nullptr, *count = nullptr, *tiles = nullptr;
  SMESH_TRY(tmp.alloc(&d_vertices, V * 12));
  SMESH_TRY(tmp.alloc(&d_faces, F * 12));
  SMESH_TRY(tmp.alloc(&box, 32));
  SMESH_TRY(tmp.alloc(&counters, 16));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&s->tris), std::max<uint64_t>(F * 48, 16)));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&s->edges), 6 * kEdgeStride * 4));
  const dim3 b(kBlock), gf((uint32_t)div_up(F, kBlock));
  const uint32_t box0[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u};
  uint32_t h_box[8], h_bad = 0;
  SMESH_HIP(hipMemcpyAsync(box, box0, 32, hipMemcpyHostToDevice, st));     // box[6]: a face index out of range was seen
  if (V) {
    SMESH_HIP(hipMemcpyAsync(d_vertices, vertices, V * 12, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pts_bbox, dim3((uint32_t)div_up(V, kBlock)), b, 0, st, d_vertices, V, box);
  }
  if (F) {
    SMESH_HIP(hipMemcpyAsync(d_faces, faces, F * 12, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pts_pack, gf, b, 0, st, d_vertices, V, d_faces, F, s->tris, box + 6);
  }
  SMESH_HIP(hipGetLastError());
  SMESH_HIP(hipMemcpyAsync(h_box, box, 32, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  h_bad = h_box[6];
  if (h_bad) return fail(SMESH_ERR_INVALID, "surface index: a face index lies outside [0, " + std::to_string(V) + ")");
  const bool any = h_box[3] != 0u;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int k = 0; k < 3 && any; k++) { lo[k] = unordered(h_box[k]); hi[k] = unordered(h_box[3 + k]); }
  Grid& g = s->grid;
  shape_grid(g, lo, hi, any, F);
  g.tris = s->tris;
  g.edges = s->edges;
  s->cells = (uint64_t)g.dims[0] * g.dims[1] * g.dims[2];
  const uint64_t n = s->cells + 1;
  SMESH_TRY(tmp.alloc(&count, n * 4));
  SMESH_TRY(tmp.alloc(&tiles, div_up(n, kScanTile) * 4));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&s->cell_start), n * 4));
  g.cell_start = s->cell_start;
  SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));
  SMESH_HIP(hipMemsetAsync(counters, 0, 16, st));
  hipLaunchKernelGGL(k_pts_edges, dim3((uint32_t)div_up(3 * kEdgeStride, kBlock)), b, 0, st, g, s->edges);
  if (F) hipLaunchKernelGGL(k_pts_count, gf, b, 0, st, g, F, count, counters);
  launch_exclusive_scan(count, s->cell_start, n, tiles, st);
  SMESH_HIP(hipGetLastError());
  uint32_t h_counters[4] = {0, 0, 0, 0};
  SMESH_HIP(hipMemcpyAsync(h_counters, counters, 16, hipMemcpyDeviceToHost, st));
  SMESH_HIP(hipStreamSynchronize(st));
  g.nlarge = h_counters[0];
  s->entries = (uint64_t)h_counters[2] | ((uint64_t)h_counters[3] << 32);
  if (s->entries >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "surface index: the cells' face lists must stay below 2^32 entries");
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&s->cell_list), std::max<uint64_t>(s->entries * 4, 16)));
  SMESH_HIP(dev_malloc(reinterpret_cast<void**>(&s->large), std::max<uint64_t>((uint64_t)g.nlarge * 4, 16)));
  g.cell_list = s->cell_list;
  g.large = s->large;
  if (F) {
    SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));      // now the fill cursors
    hipLaunchKernelGGL(k_pts_fill, gf, b, 0, st, g, F, count, s->cell_list, s->large, counters);
    SMESH_HIP(hipGetLastError());
  }
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

}  // namespace

extern "C" {

int smesh_surface_index_create(const float* vertices, uint64_t V, const int32_t* faces, uint64_t F, int device, smesh_surface_index_t** out) {
  if (!out) return fail(SMESH_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if ((F && !faces) || (V && !vertices)) return fail(SMESH_ERR_INVALID, "surface index: NULL vertices or faces");
  if (3 * F >= 0xFFFFFFFFull || V >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "surface index: 3 F and V must stay below 2^32");
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  smesh_surface_index* s = new smesh_surface_index;
  s->ctx = ctx;
  s->F = F;
  const int status = build_index(s, vertices, V, faces);
  if (status != SMESH_OK) {
    smesh_surface_index_destroy(s);
    return status;
  }
  *out = s;
  return SMESH_OK;
}

int smesh_surface_index_destroy(smesh_surface_index_t* s) {
  if (!s) return SMESH_OK;
  std::lock_guard<std::recursive_mutex> lock(s->ctx->mu);
  DeviceScope scope(s->ctx->device);
  for (void* p : {(void*)s->tris, (void*)s->edges, (void*)s->cell_start, (void*)s->cell_list, (void*)s->large})
    if (p) (void)dev_free(p);
  delete s;
  return SMESH_OK;
}

int smesh_surface_index_stats(const smesh_surface_index_t* s, uint64_t* F, uint32_t dims[3], uint64_t* entries, uint64_t* large_faces) {
  if (!s) return fail(SMESH_ERR_INVALID, "NULL surface index");
  if (F) *F = s->F;
  if (dims)
    for (int k = 0; k < 3; k++) dims[k] = (uint32_t)s->grid.dims[k];
  if (entries) *entries = s->entries;
  if (large_faces) *large_faces = s->grid.nlarge;
  return SMESH_OK;
}

int smesh_surface_index_nearest(const smesh_surface_index_t* s, const float* points, uint64_t N, int points_memkind, float max_distance,
                                int32_t* out_face, float* out_dist2, int out_memkind) {
  if (!s) return fail(SMESH_ERR_INVALID, "NULL surface index");
  if (!memkind_ok(points_memkind) || !memkind_ok(out_memkind)) return fail(SMESH_ERR_INVALID, "nearest: bad memory kind");
  if (N && (!points || !out_face)) return fail(SMESH_ERR_INVALID, "nearest: NULL points or out_face");
  if (N >= 0xFFFFFFFFull) return fail(SMESH_ERR_INVALID, "nearest: N must stay below 2^32");
  if (!(max_distance >= 0.0f)) return fail(SMESH_ERR_INVALID, "nearest: max_distance must be >= 0");
  if (N == 0) return SMESH_OK;
  DeviceCtx* ctx = s->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  TempBlocks tmp;
  const float* d_points = nullptr;
  SMESH_TRY(on_device(ctx, tmp, points, N * 12, points_memkind, &d_points));
  Out<int32_t> face;
  Out<float> dist2;      // (out_dist2 may be null: the kernels then leave it out)
  SMESH_TRY(face.init(tmp, out_face, N * 4, out_memkind));
  SMESH_TRY(dist2.init(tmp, out_dist2, N * 4, out_memkind));
  const float r2 = max_distance * max_distance;
  const dim3 b(kBlock), gn((uint32_t)div_up(N, kBlock));
  if (opt_points_grid()) {
    const uint64_t n = s->cells + 1;
    uint32_t *cell = nullptr, *count = nullptr, *start = nullptr, *tiles = nullptr, *perm = nullptr;
    SMESH_TRY(tmp.alloc(&cell, N * 4));
    SMESH_TRY(tmp.alloc(&perm, N * 4));
    SMESH_TRY(tmp.alloc(&count, n * 4));
    SMESH_TRY(tmp.alloc(&start, n * 4));
    SMESH_TRY(tmp.alloc(&tiles, div_up(n, kScanTile) * 4));
    SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));
    hipLaunchKernelGGL(k_pts_cells, gn, b, 0, st, d_points, N, s->grid, cell, count);
    launch_exclusive_scan(count, start, n, tiles, st);
    SMESH_HIP(hipMemsetAsync(count, 0, n * 4, st));      // now the fill cursors
    hipLaunchKernelGGL(k_pts_perm, gn, b, 0, st, cell, N, start, count, perm);
    hipLaunchKernelGGL(k_pts_nearest_grid, gn, b, 0, st, d_points, perm, N, s->grid, r2, face.dev, dist2.dev);
  } else {
    hipLaunchKernelGGL(k_pts_nearest_all, gn, b, 0, st, d_points, N, s->tris, s->F, r2, face.dev, dist2.dev);
  }
  SMESH_HIP(hipGetLastError());
  SMESH_TRY(face.copy_back(st));
  SMESH_TRY(dist2.copy_back(st));
  SMESH_HIP(hipStreamSynchronize(st));
  return SMESH_OK;
}

int smesh_point_gather(const float* face_rows, int rows_memkind, uint64_t F, uint32_t C, const int32_t* faces, uint64_t N, int faces_memkind,
                       int mode, float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  SMESH_TRY(check_point_gather_args(C, N, faces, faces_memkind, mode, out_rows, out_labels, out_memkind));
  if (!memkind_ok(rows_memkind)) return fail(SMESH_ERR_INVALID, "point gather: bad memory kind");
  if (F && !face_rows) return fail(SMESH_ERR_INVALID, "point gather: NULL face rows");
  int device = 0;
  if (rows_memkind == SMESH_MEM_DEVICE || faces_memkind == SMESH_MEM_DEVICE || out_memkind == SMESH_MEM_DEVICE) {
    hipPointerAttribute_t attr;      // (the device the arrays live on: the first device array names it)
    const void* p = rows_memkind == SMESH_MEM_DEVICE && face_rows ? (const void*)face_rows
                    : faces_memkind == SMESH_MEM_DEVICE && faces  ? (const void*)faces
                    : out_memkind == SMESH_MEM_DEVICE             ? (out_rows ? (const void*)out_rows : (const void*)out_labels)
                                                                  : nullptr;
    if (p && hipPointerGetAttributes(&attr, p) == hipSuccess) device = attr.device;
    else (void)hipGetLastError();
  }
  DeviceCtx* ctx = nullptr;
  SMESH_TRY(get_ctx(device, &ctx));
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  SMESH_HIP(hipSetDevice(ctx->device));
  TempBlocks tmp;
  const float* d_rows = nullptr;
  SMESH_TRY(on_device(ctx, tmp, face_rows, (size_t)F * C * 4, rows_memkind, &d_rows));
  return gather_device_rows(ctx, d_rows, F, C, faces, N, faces_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind);
}

int smesh_aggregator_point_annotations(smesh_aggregator_t* a, const int32_t* faces, uint64_t N, int faces_memkind, int mode,
                                       float dont_care_threshold, float* out_rows, int32_t* out_labels, int out_memkind) {
  if (!a) return fail(SMESH_ERR_INVALID, "NULL argument");
  SMESH_TRY(check_point_gather_args(1, N, faces, faces_memkind, mode, out_rows, out_labels, out_memkind));
  return smesh_aggregator_with_final_rows(a, [&](DeviceCtx* ctx, const float* d_rows, uint64_t P, uint32_t C) -> int {
    return gather_device_rows(ctx, d_rows, P, C, faces, N, faces_memkind, mode, dont_care_threshold, out_rows, out_labels, out_memkind);
  });
}

}  // extern "C"
