"""Labels for arbitrary points (fusion.SurfaceIndex / PointTransfer): the index build, the closest-face query for points near the
surface and for points spread over twice the bounding box, the exhaustive kernel (option "points_grid" 0) and the numpy exhaustive
route beside them, labels_device() from an aggregator, and the far cloud again with a max_distance.  Timed by a host clock around smesh_synchronize; medians of REPS repeats
with min - max, after one warm-up call.
usage: python tools/point_transfer_bench.py [output file, default profiles/point_transfer_bench.json]

Rules fixed before the run:
  * a case whose warm-up call takes longer than SLOW_S seconds is timed once more instead of REPS times, and says so ("repeats": 1);
  * the 1 M-point case of a distribution is skipped (and listed under "not_measured") when four times the 250 k median exceeds SLOW_S;
  * the numpy route runs once.
There is one form of the query kernel (one lane per point, no LDS staging), so there is nothing to decide between."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from semantic_meshes_amd import _lib, device, fusion, synth          # noqa: E402

REPS = 7
SLOW_S = 6.0


def timed(call):
    """dict(median_ms, min_ms, max_ms, repeats) of `call`, each run bracketed by smesh_synchronize."""
    def once():
        _lib.synchronize(0)
        t0 = time.perf_counter()
        out = call()
        _lib.synchronize(0)
        ms = 1e3 * (time.perf_counter() - t0)
        del out
        return ms
    warm = once()
    ms = [once() for _ in range(REPS if warm <= 1e3 * SLOW_S else 1)]
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms), warm_up_ms=warm)


def surface_points(rng, mesh, n, jitter):
    pick = rng.integers(0, len(mesh.faces), n)
    w = rng.dirichlet(np.ones(3), n)[:, :, None]
    return ((mesh.vertices[mesh.faces[pick]] * w).sum(axis=1) + rng.normal(0.0, jitter, (n, 3))).astype(np.float32)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "point_transfer_bench.json")
    mesh = synth.grid_mesh(1000, 500)                                # the 1 M-triangle mesh of synth (cfg2)
    F = len(mesh.faces)
    v = mesh.vertices
    edge = float(np.mean([np.linalg.norm(v[mesh.faces[:, a]] - v[mesh.faces[:, b]], axis=1).mean() for a, b in ((0, 1), (1, 2), (2, 0))]))
    lo, hi = v.min(axis=0), v.max(axis=0)
    rng = np.random.default_rng(0)
    result = dict(tool="tools/point_transfer_bench.py", timing="host clock around smesh_synchronize; median of %d after a warm-up" % REPS,
                  faces=F, vertices=len(v), mean_edge=edge, not_measured=[])
    result["index_build"] = timed(lambda: fusion.SurfaceIndex.from_mesh(mesh))
    index = fusion.SurfaceIndex.from_mesh(mesh)
    result["index"] = index.stats()
    clouds = {}

    def save():
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    def run_cloud(name, draw):
        last = None
        for n in (250000, 1000000):
            key = "nearest_%s_%dk" % (name, n // 1000)
            if last is not None and 4 * last["median_ms"] > 1e3 * SLOW_S:
                result["not_measured"].append(key + ": four times the 250 k median exceeds %g s" % SLOW_S)
                continue
            pts = device.to_device(draw(n))
            last = timed(lambda: index.nearest_device(pts))
            last["points"] = n
            last["ns_per_point"] = 1e6 * last["median_ms"] / n
            faces, dist2 = index.nearest_device(pts)
            last["mean_distance_in_edges"] = float(np.sqrt(dist2.numpy().astype(np.float64)).mean() / edge)
            result[key] = last
            clouds[key] = pts
            print(key, last, flush=True)
        save()

    run_cloud("surface", lambda n: surface_points(rng, mesh, n, edge))
    # the exhaustive kernel on 4096 of the surface points, per point; its answers beside the grid's
    few = device.to_device(clouds["nearest_surface_250k"].numpy()[:4096])
    grid_faces, grid_dist2 = (a.numpy() for a in index.nearest_device(few))
    _lib.set_option("points_grid", 0)
    try:
        t = timed(lambda: index.nearest_device(few))
        all_faces, all_dist2 = (a.numpy() for a in index.nearest_device(few))
    finally:
        _lib.set_option("points_grid", 1)
    t["points"], t["ns_per_point"] = 4096, 1e6 * t["median_ms"] / 4096
    t["equal_to_grid"] = bool(np.array_equal(grid_faces, all_faces) and np.array_equal(grid_dist2.view(np.uint32), all_dist2.view(np.uint32)))
    result["nearest_exhaustive_4096"] = t
    print("exhaustive", t, flush=True)
    # labels from an aggregator
    pt = fusion.PointTransfer(index, clouds.get("nearest_surface_1000k", clouds["nearest_surface_250k"]))
    for C in (19, 40):
        agg = fusion.MeshAggregator(F, C)
        for r0 in range(0, F, 250000):
            raw = rng.random((min(250000, F - r0), C), dtype=np.float32)
            raw[rng.random(len(raw)) < 0.3] = 0.0
            agg.set_raw_rows(r0, raw)
        t = timed(lambda: pt.labels_device(agg))
        t["points"], t["classes"] = pt.num_points, C
        result["labels_device_C%d" % C] = t
        g = timed(agg.get_device)
        result["get_device_C%d" % C] = g
        del agg
        print("labels C=%d" % C, t, flush=True)
    # numpy, exhaustive, once
    import points_ref
    host_pts = clouds["nearest_surface_250k"].numpy()[:256]
    t0 = time.perf_counter()
    ref_faces, ref_dist2 = points_ref.nearest(v, mesh.faces, host_pts, chunk=4)
    s = time.perf_counter() - t0
    result["numpy_exhaustive_256"] = dict(seconds=s, points=256, ms_per_point=1e3 * s / 256, repeats=1,
                                          equal_to_grid=bool(np.array_equal(ref_faces, grid_faces[:256]) and
                                                             np.array_equal(ref_dist2.view(np.uint32), grid_dist2[:256].view(np.uint32))))
    print("numpy", result["numpy_exhaustive_256"], flush=True)
    save()
    # last, because it is the slow one: points spread over twice the bounding box walk most of the grid
    run_cloud("uniform_2x_box", lambda n: (0.5 * (lo + hi) + 2.0 * (hi - lo) * (rng.random((n, 3)) - 0.5)).astype(np.float32))
    # ... and what a max_distance of ten mean edge lengths makes of that cloud: the walk ends once the bound exceeds it
    pts = clouds["nearest_uniform_2x_box_250k"]
    t = timed(lambda: index.nearest_device(pts, max_distance=10.0 * edge))
    t["points"], t["ns_per_point"], t["max_distance_in_edges"] = 250000, 1e6 * t["median_ms"] / 250000, 10.0
    t["points_with_a_face"] = int((index.nearest_device(pts, max_distance=10.0 * edge)[0].numpy() >= 0).sum())
    result["nearest_uniform_2x_box_250k_max_distance"] = t
    print("max_distance", t, flush=True)
    save()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
