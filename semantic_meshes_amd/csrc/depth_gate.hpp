// depth_gate.hpp -- what raster.hip's gated view driver, depth_weights.hip (include/smesh_depth.h), view_weights.hip
// (include/smesh_view_weights.h) and edge_weights.hip (include/smesh_edge_gate.h) share.
#pragma once

#include <functional>
#include <mutex>

#include "common.hpp"
#include "view_input.hpp"
#include "../../include/smesh_depth.h"

namespace smesh {

// Device scratch of the gated entry points, owned by the renderer: the weights planes of a group of views, the staged host sensor
// images of that group, and the group's counts (the depth gate's; the view weights'; the edge gate's).  Everything that writes or
// reads them is ordered on the context's main stream.
struct DepthScratch {
  Scratch w, sensor, counts, view_counts, edge_counts;
  void release() { w.release(); sensor.release(); counts.release(); view_counts.release(); edge_counts.release(); }
};

// One view of a group between the rasteriser and the fusion launch: its depth plane, the caller's weights (or null) and the plane the
// gate writes, all dense (W,H) float32 in device memory; the view's index plane (dense uint32 (W,H)) and its camera, where the driver
// knows them (smesh_renderer_fuse_views_gated does).
struct GatedView {
  const float* depth;
  const float* w_in;
  float* w_out;
  uint64_t W, H;
  const uint32_t* idx = nullptr;
  const smesh_camera_t* cam = nullptr;
};

// Queues the weights of views first .. first + m - 1 (m <= kGroup) on the context's main stream; called with the renderer, the
// aggregator and the context locked and the device current.
using GateFn = std::function<int(DeviceCtx* ctx, DepthScratch& scratch, uint64_t first, int m, const GatedView* views)>;

// The sensor images and the gate of a depth-gated call (depth_weights.hip), for callers that gate planes another stage wrote.
struct DepthGateCall {
  const void* const* sensors;   // one per view of the call
  int dtype, memkind;
  const int64_t* strides;       // or null: dense
  uint64_t w, h;
  smesh_depth_gate_t gate;
};
// What every entry point of smesh_depth.h refuses about the sensor images and the gate.
int depth_gate_check(int dtype, const int64_t* strides, int memkind, uint64_t w, uint64_t h, const smesh_depth_gate_t* gate);
// k_depth_weights for views first .. first + m - 1 of `call`; `counts_host`: [m][4] or null (asking makes the call wait).
int depth_gate_group(DeviceCtx* ctx, DepthScratch& scratch, const GatedView* views, const DepthGateCall& call, uint64_t first, int m,
                     uint64_t* counts_host);
// The ViewInput of a SMESH_DEPTH_IMG_* image kind for `aggregator` (image pointer unset), or SMESH_ERR_INVALID.
int depth_image_input(smesh_aggregator* aggregator, int image_kind, ViewInput* in);

// What view_weights.hip needs of a renderer (raster.hip): its mesh as the rasteriser processes it -- `prim_id[p]` is the id the index
// plane holds for the triangle at position p, null: p itself -- and the slot of the face-normals table, float32 [F][4] indexed by
// that id, null until first use; the slot is read and written with `mu` and the context locked.
struct RendererMesh {
  DeviceCtx* ctx;
  uint64_t V, F;
  const float* verts;
  const int32_t* faces;
  const uint32_t* prim_id;
  bool texels;
  float** normals;
  std::mutex* mu;
};

}  // namespace smesh

struct smesh_aggregator;
struct smesh_renderer;
// raster.hip.  smesh_fuse_views for `n` views whose dense images (`in`: F32, HALF or LABELS; images[i]: view i's) and weights are in
// DEVICE memory, every view's weights plane computed by `gate` from the depth plane of its render: per group of up to eight views,
// each view is rasterised into its slot with its depth plane (main stream), `gate` is called once, and the group is fused from the
// planes it wrote -- by the multi-view launches of smesh_fuse_views where they serve the renderer and the aggregator, else view by view.
int smesh_renderer_fuse_views_gated(smesh_renderer* r, smesh_aggregator* a, const smesh_camera_t* cams, uint64_t n, const smesh::ViewInput& in,
                                    const void* const* images, const float* const* weights, const smesh::GateFn& gate);
// raster.hip
int smesh_renderer_mesh(smesh_renderer* r, smesh::RendererMesh* out);

struct smesh_view_weights_spec;
namespace smesh {
// view_weights.hip, for callers that run another stage behind the view weights (edge_weights.hip).
// What every entry point of smesh_view_weights.h refuses about the spec and the renderer; fills `mesh`.
int view_weights_check(smesh_renderer* r, const smesh_view_weights_spec* spec, RendererMesh* mesh);
// k_view_weights for a group of m views; `counts_host`: [m][4] or null (asking makes the call wait).
int view_weights_group(DeviceCtx* ctx, const RendererMesh& mesh, DepthScratch& scratch, const GatedView* views, int m,
                       const smesh_view_weights_spec& spec, uint64_t* counts_host);
}  // namespace smesh
