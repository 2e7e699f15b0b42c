// depth_gate.hpp -- what raster.hip's gated view driver and depth_weights.hip (include/smesh_depth.h) share.
#pragma once

#include <functional>

#include "common.hpp"
#include "view_input.hpp"

namespace smesh {

// Device scratch of the gated entry points, owned by the renderer: the weights planes of a group of views, the staged host sensor
// images of that group, and the group's counts.  Everything that writes or reads them is ordered on the context's main stream.
struct DepthScratch {
  Scratch w, sensor, counts;
  void release() { w.release(); sensor.release(); counts.release(); }
};

// One view of a group between the rasteriser and the fusion launch: its depth plane, the caller's weights (or null) and the plane the
// gate writes, all dense (W,H) float32 in device memory.
struct GatedView {
  const float* depth;
  const float* w_in;
  float* w_out;
  uint64_t W, H;
};

// Queues the weights of views first .. first + m - 1 (m <= kGroup) on the context's main stream; called with the renderer, the
// aggregator and the context locked and the device current.
using GateFn = std::function<int(DeviceCtx* ctx, DepthScratch& scratch, uint64_t first, int m, const GatedView* views)>;

}  // namespace smesh

struct smesh_aggregator;
struct smesh_renderer;
// raster.hip.  smesh_fuse_views for `n` views whose dense images (`in`: F32, HALF or LABELS; images[i]: view i's) and weights are in
// DEVICE memory, every view's weights plane computed by `gate` from the depth plane of its render: per group of up to eight views,
// each view is rasterised into its slot with its depth plane (main stream), `gate` is called once, and the group is fused from the
// planes it wrote -- by the multi-view launches of smesh_fuse_views where they serve the renderer and the aggregator, else view by view.
int smesh_renderer_fuse_views_gated(smesh_renderer* r, smesh_aggregator* a, const smesh_camera_t* cams, uint64_t n, const smesh::ViewInput& in,
                                    const void* const* images, const float* const* weights, const smesh::GateFn& gate);
