"""fuse_views gated by sensor depth (include/smesh_depth.h) at the two geometries the reference's scripts use, on the 1 M-triangle mesh:
16 views per call, medians of 7 repeats with min - max after a warm-up that is not timed; a leg's time is a host clock around
smesh_synchronize for the call, per view.  All legs run in one process.
  scannet     640 x 480 uint16 millimetres -> 1296 x 968, 40 classes
  1080p       1920 x 1080 float32 metres at full size, 19 classes
The device sensor images are decoded (h,w) images passed as their transposed (w,h) views.  Each is the render's own depth with a
band of the image moved half a metre nearer (an occluder), and holes.
  a  fuse_views(sensor_depths=, depth_gate=)                                   (k_depth_weights between rasteriser and fusion)
  b  fuse_views with weights planes computed beforehand                        (the floor: what fusing with weights costs)
  c  plain fuse_views                                                          (no weights at all)
  d  per view: render() + depth_weights_device() + add()                       (the reference's loop, weights on the device)
  e  per view: render(), depth to the host, numpy, weights back, add()         (the only route before this entry point)
The accumulators of a, b, d and e are compared in bits once per case.
`python tools/depth_gate_bench.py kernel <geometry>` runs leg a five times and nothing else: the run to put under a kernel trace
for k_depth_weights' own duration; `python tools/depth_gate_bench.py merge <stats csv> <geometry> [output file]` adds that duration to
the output file with the bytes the kernel has to move as a share of 8 TB/s.
usage: python tools/depth_gate_bench.py [output file, default profiles/depth_gate_bench.json]"""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, fusion, render, synth          # noqa: E402
from semantic_meshes_amd.device import to_device                     # noqa: E402

VIEWS, REPS = 16, 7
HBM_BYTES_PER_S = 8e12
GEOMETRIES = ({"name": "scannet", "source": (640, 480), "target": (1296, 968), "classes": 40, "dtype": "uint16", "abs_tol": 0.05},
              {"name": "1080p", "source": (1920, 1080), "target": (1920, 1080), "classes": 19, "dtype": "float32", "abs_tol": 0.05})
DEFAULT_OUT = os.path.join(ROOT, "profiles", "depth_gate_bench.json")


def wall_ms(run):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    run()
    _lib.synchronize(0)
    return 1e3 * (time.perf_counter() - t0) / VIEWS


def measure(run, warm=2):
    for _ in range(warm):
        run()
    _lib.synchronize(0)
    return [wall_ms(run) for _ in range(REPS)]


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def axis_index(n, N):
    return ((2 * np.arange(N, dtype=np.int64) + 1) * n) // (2 * N)


def numpy_weights(depth, sensor, scale, abs_tol):
    """The rule of smesh_depth.h as a user writes it in numpy (rel_tol 0, no max_depth, missing kept)."""
    W, H = depth.shape
    w, h = sensor.shape
    raw = sensor if (w, h) == (W, H) else sensor[axis_index(w, W)[:, None], axis_index(h, H)[None, :]]
    d_s = raw.astype(np.float32) * np.float32(scale)
    with np.errstate(invalid="ignore"):
        missing = (raw == 0) if raw.dtype.kind == "u" else (~(raw > 0) | ~np.isfinite(raw))
        ok = np.isfinite(depth) & (missing | (np.abs(depth - d_s) <= np.float32(abs_tol)))
    return ok.astype(np.float32)


def setup(g, r):
    (w, h), (W, H), C, dt = g["source"], g["target"], g["classes"], np.dtype(g["dtype"])
    rng = np.random.default_rng(11)
    cams = [synth.ring_camera(k, VIEWS, W, H) for k in range(VIEWS)]
    decoded = []
    for cam in cams:
        depth = np.asarray(r.render(cam)[1])                          # (W,H) float32, +inf for background
        d = depth[axis_index(W, w)[:, None], axis_index(H, h)[None, :]].astype(np.float64)
        d[w // 3: w // 2, :] -= 0.5                                    # something the mesh does not hold, in front of it
        d[rng.random((w, h)) < 0.03] = 0.0                             # holes
        d = np.where(np.isfinite(d), d, 0.0)
        s = np.rint(1000.0 * d).astype(np.uint16) if dt == np.uint16 else d.astype(np.float32)
        decoded.append(np.ascontiguousarray(s.T))                      # (h,w): as a decoder leaves it
    probs = [synth.device_probs(W, H, C, 100 + k) for k in range(VIEWS)]
    return cams, decoded, probs


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    result = {"tool": "tools/depth_gate_bench.py", "views_per_call": VIEWS, "reps": REPS, "mesh_triangles": P,
              "timing": "host clock around smesh_synchronize for one call (a, b, c) or one loop (d, e) of %d views, microseconds per view" % VIEWS,
              "cases": []}
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (w, h), (W, H), C, dt = g["source"], g["target"], g["classes"], np.dtype(g["dtype"])
        cams, decoded, probs = setup(g, r)
        host = [x.T for x in decoded]
        dev = [to_device(x).T for x in decoded]
        gate = fusion.DepthGate(g["abs_tol"])
        scale = gate.scale_for(dt)
        case = {"geometry": g["name"], "source": [w, h], "target": [W, H], "classes": C, "dtype": dt.name, "abs_tol": g["abs_tol"]}

        def leg_d(a):
            for k, cam in enumerate(cams):
                idx, depth = r.render(cam)
                a.add(idx, probs[k], fusion.depth_weights_device(depth, dev[k], gate))

        def leg_e(a):
            for k, cam in enumerate(cams):
                idx, depth = r.render(cam)
                a.add(idx, probs[k], to_device(numpy_weights(np.asarray(depth), host[k], scale, g["abs_tol"])))

        # the legs give the same sums: checked once per case
        before = _lib.get_option("depth_weights_launches")
        a = fusion.MeshAggregator(P, C)
        counts = a.fuse_views(r, cams, probs, sensor_depths=dev, depth_gate=gate, depth_stats=True)
        if _lib.get_option("depth_weights_launches") - before != VIEWS // 8:
            raise SystemExit("leg a did not launch k_depth_weights once per group (%s)" % g["name"])
        case["kernel"] = _lib.last_fuse_kernel()
        sums = [a.get_raw().view(np.uint32)]
        case["counts_visible_far_missing_inconsistent"] = [int(x) for x in counts.sum(axis=0)]
        planes = [fusion.depth_weights_device(r.render(cam)[1], dev[k], gate) for k, cam in enumerate(cams)]
        for leg in (lambda a: a.fuse_views(r, cams, probs, planes), leg_d, leg_e):
            a = fusion.MeshAggregator(P, C)
            leg(a)
            sums.append(a.get_raw().view(np.uint32))
        case["bit_equal_a_b_d_e"] = [bool(np.array_equal(sums[0], s)) for s in sums[1:]]
        del a, sums

        agg = fusion.MeshAggregator(P, C)
        case["a"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, sensor_depths=dev, depth_gate=gate)))
        case["b"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, planes)))
        case["c"] = stats(measure(lambda: agg.fuse_views(r, cams, probs)))
        case["d"] = stats(measure(lambda: leg_d(agg)))
        case["e"] = stats(measure(lambda: leg_e(agg), warm=1))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del dev, planes, probs, agg
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def kernel_run(name):
    g = next(x for x in GEOMETRIES if x["name"] == name)
    mesh = synth.grid_mesh(1000, 500)
    r = render.triangles(mesh)
    cams, decoded, probs = setup(g, r)
    dev = [to_device(x).T for x in decoded]
    agg = fusion.MeshAggregator(len(mesh.faces), g["classes"])
    gate = fusion.DepthGate(g["abs_tol"])
    for _ in range(5):
        agg.fuse_views(r, cams, probs, sensor_depths=dev, depth_gate=gate)
    _lib.synchronize(0)


def merge(csv_path, name, out_path):
    g = next(x for x in GEOMETRIES if x["name"] == name)
    rows = [row for row in csv.DictReader(open(csv_path)) if "k_depth_weights" in row.get("Name", "")]
    if not rows:
        raise SystemExit("no k_depth_weights row in %s" % csv_path)
    calls = sum(int(row["Calls"]) for row in rows)
    total_ns = sum(float(row["TotalDurationNs"]) for row in rows)
    (w, h), (W, H) = g["source"], g["target"]
    per_pixel = 8.0 + np.dtype(g["dtype"]).itemsize * (w * h) / float(W * H)      # depth in, weights out, the sensor image once
    launch_bytes = 8 * W * H * per_pixel
    avg_us = total_ns / calls / 1e3
    result = json.load(open(out_path))
    for case in result["cases"]:
        if case["geometry"] == name:
            case["k_depth_weights"] = {"launches": calls, "views_per_launch": 8, "avg_us_per_launch": avg_us, "us_per_view": avg_us / 8,
                                       "needed_bytes_per_pixel": per_pixel, "needed_bytes_per_launch": launch_bytes,
                                       "share_of_8_TB_per_s": launch_bytes / (avg_us * 1e-6) / HBM_BYTES_PER_S,
                                       "source": "rocprofv3 --kernel-trace --stats, a run of its own (5 calls of leg a)"}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("merged", name, "into", out_path)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "kernel":
        kernel_run(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else DEFAULT_OUT)
    else:
        main()
