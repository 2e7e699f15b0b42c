"""fuse_views weighted by viewing geometry (include/smesh_view_weights.h) at the two geometries the reference's scripts use, on the
1 M-triangle mesh: 16 views per call, medians of 7 repeats with min - max after a warm-up that is not timed; a leg's time is a host
clock around smesh_synchronize for the call, per view.  All legs run in one process.
  scannet     1296 x 968, 40 classes
  1080p       1920 x 1080, 19 classes
The spec is ViewWeights(power=2, min_cos=0.1, two_sided=True, falloff_depth=6.0).
  a  fuse_views(view_weights=)                                                 (k_view_weights between rasteriser and fusion)
  b  fuse_views with weights planes computed beforehand                        (the floor: what fusing with weights costs)
  c  plain fuse_views                                                          (no weights at all)
  d  per view: render() + view_weights_device() + add()                        (the reference's loop, weights on the device)
  e  per view: render(), index and depth planes to the host, the numpy restatement (tests/view_weights_ref.py), weights back, add()
                                                                               (the only route before this entry point)
  f  a with a depth gate as well (full-size uint16 sensor images), against the depth-gated call alone
The accumulators of a, b, d and e are compared in bits once per case, and the tool stops if they differ.
`python tools/view_weights_bench.py kernel <geometry>` runs leg a five times and nothing else: the run to put under a kernel trace
for k_view_weights' own duration; `python tools/view_weights_bench.py merge <stats csv> <geometry> [output file]` adds that duration
(and k_depth_weights', where the trace holds it) to the output file with the bytes the kernel has to move as a share of 8 TB/s.
usage: python tools/view_weights_bench.py [output file, default profiles/view_weights_bench.json]"""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from semantic_meshes_amd import _lib, fusion, render, synth          # noqa: E402
from semantic_meshes_amd.device import to_device                     # noqa: E402
import view_weights_ref as vw                                        # noqa: E402

VIEWS, REPS = 16, 7
HBM_BYTES_PER_S = 8e12
SPEC = dict(power=2, min_cos=0.1, two_sided=True, max_depth=None, falloff_depth=6.0)
GEOMETRIES = ({"name": "scannet", "target": (1296, 968), "classes": 40}, {"name": "1080p", "target": (1920, 1080), "classes": 19})
DEFAULT_OUT = os.path.join(ROOT, "profiles", "view_weights_bench.json")


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


def setup(g, r):
    (W, H), C = g["target"], g["classes"]
    cams = [synth.ring_camera(k, VIEWS, W, H) for k in range(VIEWS)]
    sensors = []
    for cam in cams:
        depth = np.asarray(r.render(cam)[1]).astype(np.float64)        # (W,H), +inf for background
        depth[W // 3: W // 2, :] -= 0.5                                 # something the mesh does not hold, in front of it
        sensors.append(to_device(np.rint(1000.0 * np.where(np.isfinite(depth), depth, 0.0)).astype(np.uint16)))
    probs = [synth.device_probs(W, H, C, 100 + k) for k in range(VIEWS)]
    return cams, sensors, probs


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    normals = vw.face_normals(mesh.vertices, mesh.faces)
    spec, s = fusion.ViewWeights(**SPEC), vw.spec(**SPEC)
    gate = fusion.DepthGate(0.05)
    result = {"tool": "tools/view_weights_bench.py", "views_per_call": VIEWS, "reps": REPS, "mesh_triangles": P, "spec": repr(spec),
              "timing": "host clock around smesh_synchronize for one call (a, b, c, f) or one loop (d, e) of %d views, microseconds per view" % VIEWS,
              "cases": []}
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (W, H), C = g["target"], g["classes"]
        cams, sensors, probs = setup(g, r)
        case = {"geometry": g["name"], "target": [W, H], "classes": C}

        def leg_d(a):
            for k, cam in enumerate(cams):
                idx, depth = r.render(cam)
                a.add(idx, probs[k], fusion.view_weights_device(r, cam, idx, depth, spec))

        def leg_e(a):
            for k, cam in enumerate(cams):
                idx, depth = r.render(cam)
                a.add(idx, probs[k], to_device(vw.weights(cam, normals, np.asarray(idx), np.asarray(depth), s)[0]))

        # the legs give the same sums: checked once per case
        before = _lib.get_option("view_weights_launches")
        a = fusion.MeshAggregator(P, C)
        counts = a.fuse_views(r, cams, probs, view_weights=spec, view_stats=True)
        if _lib.get_option("view_weights_launches") - before != VIEWS // 8:
            raise SystemExit("leg a did not launch k_view_weights once per group (%s)" % g["name"])
        case["kernel"] = _lib.last_fuse_kernel()
        sums = [a.get_raw().view(np.uint32)]
        case["counts_visible_far_grazing_backfacing"] = [int(x) for x in counts.sum(axis=0)]
        planes = []
        for cam in cams:
            idx, depth = r.render(cam)
            planes.append(fusion.view_weights_device(r, cam, idx, depth, spec))
        for leg in (lambda a: a.fuse_views(r, cams, probs, planes), leg_d, leg_e):
            a = fusion.MeshAggregator(P, C)
            leg(a)
            sums.append(a.get_raw().view(np.uint32))
        case["bit_equal_a_b_d_e"] = [bool(np.array_equal(sums[0], x)) for x in sums[1:]]
        if not all(case["bit_equal_a_b_d_e"]):
            raise SystemExit("the accumulators of legs a, b, d, e differ (%s): %s" % (g["name"], case["bit_equal_a_b_d_e"]))
        del a, sums

        agg = fusion.MeshAggregator(P, C)
        case["a"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, view_weights=spec)))
        case["b"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, planes)))
        case["c"] = stats(measure(lambda: agg.fuse_views(r, cams, probs)))
        case["d"] = stats(measure(lambda: leg_d(agg)))
        case["e"] = stats(measure(lambda: leg_e(agg), warm=1))
        case["f_view_weights_and_depth_gate"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, sensor_depths=sensors, depth_gate=gate, view_weights=spec)))
        case["f_depth_gate_alone"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, sensor_depths=sensors, depth_gate=gate)))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del sensors, planes, probs, agg
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def kernel_run(name):
    g = next(x for x in GEOMETRIES if x["name"] == name)
    mesh = synth.grid_mesh(1000, 500)
    r = render.triangles(mesh)
    cams, sensors, probs = setup(g, r)
    agg = fusion.MeshAggregator(len(mesh.faces), g["classes"])
    spec, gate = fusion.ViewWeights(**SPEC), fusion.DepthGate(0.05)
    for _ in range(5):
        agg.fuse_views(r, cams, probs, view_weights=spec)
    for _ in range(5):      # the yardstick of the same session: k_depth_weights on full-size uint16 sensor images
        agg.fuse_views(r, cams, probs, sensor_depths=sensors, depth_gate=gate)
    _lib.synchronize(0)


def merge(csv_path, name, out_path):
    g = next(x for x in GEOMETRIES if x["name"] == name)
    W, H = g["target"]
    table = list(csv.DictReader(open(csv_path)))
    result = json.load(open(out_path))
    # index and depth in, weights out (no weights-in plane in leg a), and the normals of the faces a view shows: at most one 16-byte
    # row per pixel, at least one per visible face -- the share below counts the planes alone, the lower bound
    for kernel, per_pixel in (("k_view_weights", 12.0), ("k_depth_weights", 10.0)):
        rows = [row for row in table if kernel in row.get("Name", "")]
        if not rows:
            if kernel == "k_view_weights":
                raise SystemExit("no k_view_weights row in %s" % csv_path)
            continue
        calls = sum(int(row["Calls"]) for row in rows)
        avg_us = sum(float(row["TotalDurationNs"]) for row in rows) / calls / 1e3
        launch_bytes = 8 * W * H * per_pixel
        for case in result["cases"]:
            if case["geometry"] == name:
                case[kernel] = {"launches": calls, "views_per_launch": 8, "avg_us_per_launch": avg_us, "us_per_view": avg_us / 8,
                                "needed_bytes_per_pixel": per_pixel, "needed_bytes_per_launch": launch_bytes,
                                "share_of_8_TB_per_s": launch_bytes / (avg_us * 1e-6) / HBM_BYTES_PER_S,
                                "source": "rocprofv3 --kernel-trace --stats, a run of its own (5 calls of leg a, 5 depth-gated calls)"}
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
