"""fuse_views gated at occlusion edges (include/smesh_edge_gate.h) at the two geometries the reference's scripts use, on the
1 M-triangle mesh: 16 views per call, medians of 7 repeats with min - max after a warm-up that is not timed; a leg's time is a host
clock around smesh_synchronize for the call, per view.  All legs of a case run in one process.
  scannet     1296 x 968, 40 classes
  1080p       1920 x 1080, 19 classes
The gate is EdgeGate(radius, abs_tol=0.05, rel_tol=0.01, behind=True, front=True, silhouette=True), radius 2 and radius 8.
  a  fuse_views(edge_gate=)                                                    (k_edge_weights between rasteriser and fusion)
  b  fuse_views with weights planes computed beforehand                        (the floor: what fusing with weights costs)
  c  plain fuse_views                                                          (no weights at all)
  d  per view: render() + edge_weights_device() + add()                        (the reference's loop, weights on the device)
  e  per view: render(), the depth plane to the host, the numpy restatement (tests/edge_gate_ref.py), weights back, add()
                                                                               (the only route before this entry point)
  f  all three stages: view weights, edge gate and depth gate (full-size uint16 sensor images)
The accumulators of a, b, d and e are compared in bits once per case, and the tool stops if they differ.
`python tools/edge_gate_bench.py kernel <geometry>` runs leg a five times at each radius and five depth-gated calls on full-size
float32 sensor planes and nothing else: the run to put under a kernel trace for k_edge_weights' own duration beside its yardstick
k_depth_weights; `python tools/edge_gate_bench.py merge <kernel trace csv> <geometry> [output file]` adds them to the output file
with the bytes the kernel has to move (8 per pixel: depth in, weights out; 12 with a weights-in plane) as a share of 8 TB/s.
`python tools/edge_gate_bench.py form` queues smesh_edge_weights alone on a 1920 x 1080 plane, twenty calls at radius 1, then at 2,
then at 8, and nothing else; `python tools/edge_gate_bench.py merge_form <kernel trace csv> <label> [output file]` stores the
kernel's durations from the trace of such a run under `label`: the measurement behind ONE decision, whose rule is fixed here before
any run --
    the kernel takes its window separably (along y, then along x).  A direct (2 r + 1)^2 window over the same LDS tile is the simpler
    code at small radii.  The tree keeps a single form: the separable one stays unless the direct one is faster beyond the runs'
    min - max spread at radius 1 or radius 2; in a tie the simpler code would win only if it could serve every radius, which at
    radius 8 (289 reads per pixel) it cannot, so a tie keeps the separable form.
The direct form is not kept in the tree; it is measured from a development build of the library selected with SMESH_LIB_PATH.
Leg e uses edge_gate_ref's separable numpy form (the brute-force one takes minutes per view at radius 8; tests/test_edge_gate_host.py
holds the two to the same bits) and is timed over the first four views, three repeats.
usage: python tools/edge_gate_bench.py [output file, default profiles/edge_gate_bench.json]"""
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
import edge_gate_ref as eg                                           # noqa: E402

VIEWS, REPS = 16, 7
HBM_BYTES_PER_S = 8e12
RADII = (2, 8)
GATE = dict(abs_tol=0.05, rel_tol=0.01, behind=True, front=True, silhouette=True)
VSPEC = dict(power=2, min_cos=0.1, two_sided=True, max_depth=None, falloff_depth=6.0)
GEOMETRIES = ({"name": "scannet", "target": (1296, 968), "classes": 40}, {"name": "1080p", "target": (1920, 1080), "classes": 19})
DEFAULT_OUT = os.path.join(ROOT, "profiles", "edge_gate_bench.json")


def wall_ms(run, per=VIEWS):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    run()
    _lib.synchronize(0)
    return 1e3 * (time.perf_counter() - t0) / per


def measure(run, warm=2, per=VIEWS):
    for _ in range(warm):
        run()
    _lib.synchronize(0)
    return [wall_ms(run, per) for _ in range(REPS)]


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def setup(g, r, sensor_dtype=np.uint16):
    (W, H), C = g["target"], g["classes"]
    cams = [synth.ring_camera(k, VIEWS, W, H) for k in range(VIEWS)]
    sensors = []
    for cam in cams:
        depth = np.asarray(r.render(cam)[1]).astype(np.float64)        # (W,H), +inf for background
        depth[W // 3: W // 2, :] -= 0.5                                 # something the mesh does not hold, in front of it
        depth = np.where(np.isfinite(depth), depth, 0.0)
        sensors.append(to_device(np.rint(1000.0 * depth).astype(np.uint16) if sensor_dtype == np.uint16 else depth.astype(np.float32)))
    probs = [synth.device_probs(W, H, C, 100 + k) for k in range(VIEWS)]
    return cams, sensors, probs


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    dgate, vspec = fusion.DepthGate(0.05), fusion.ViewWeights(**VSPEC)
    result = {"tool": "tools/edge_gate_bench.py", "views_per_call": VIEWS, "reps": REPS, "mesh_triangles": P,
              "timing": "host clock around smesh_synchronize for one call (a, b, c, f) or one loop (d, e) of %d views, microseconds per view" % VIEWS,
              "cases": []}
    if os.path.exists(out_path):               # (keep what the `merge` and `form` runs stored)
        result.update({k: v for k, v in json.load(open(out_path)).items() if k in ("form", "kernel_trace")})
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (W, H), C = g["target"], g["classes"]
        cams, sensors, probs = setup(g, r)
        for radius in RADII:
            gate, gref = fusion.EdgeGate(radius, **GATE), eg.gate(radius, **GATE)
            case = {"geometry": g["name"], "target": [W, H], "classes": C, "radius": radius, "gate": repr(gate)}

            def leg_d(a):
                for k, cam in enumerate(cams):
                    idx, depth = r.render(cam)
                    a.add(idx, probs[k], fusion.edge_weights_device(depth, gate))

            def leg_e(a, views=VIEWS):
                for k, cam in enumerate(cams[:views]):
                    idx, depth = r.render(cam)
                    a.add(idx, probs[k], to_device(eg.weights_separable(np.asarray(depth), gref)[0]))

            # the legs give the same sums: checked once per case
            before = _lib.get_option("edge_weights_launches")
            a = fusion.MeshAggregator(P, C)
            counts = a.fuse_views(r, cams, probs, edge_gate=gate, edge_stats=True)
            if _lib.get_option("edge_weights_launches") - before != VIEWS // 8:
                raise SystemExit("leg a did not launch k_edge_weights once per group (%s)" % g["name"])
            case["kernel"] = _lib.last_fuse_kernel()
            sums = [a.get_raw().view(np.uint32)]
            case["counts_visible_behind_front_silhouette"] = [int(x) for x in counts.sum(axis=0)]
            planes = [fusion.edge_weights_device(r.render(cam)[1], gate) for cam in cams]
            for leg in (lambda a: a.fuse_views(r, cams, probs, planes), leg_d, leg_e):
                a = fusion.MeshAggregator(P, C)
                leg(a)
                sums.append(a.get_raw().view(np.uint32))
            case["bit_equal_a_b_d_e"] = [bool(np.array_equal(sums[0], x)) for x in sums[1:]]
            if not all(case["bit_equal_a_b_d_e"]):
                raise SystemExit("the accumulators of legs a, b, d, e differ (%s): %s" % (g["name"], case["bit_equal_a_b_d_e"]))
            del a, sums

            agg = fusion.MeshAggregator(P, C)
            case["a"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, edge_gate=gate)))
            case["b"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, planes)))
            case["c"] = stats(measure(lambda: agg.fuse_views(r, cams, probs)))
            case["d"] = stats(measure(lambda: leg_d(agg)))
            case["e"] = stats([wall_ms(lambda: leg_e(agg, 4), per=4) for _ in range(3)])      # (host numpy: four views, three repeats)
            case["e_views_reps"] = [4, 3]
            case["f_all_three_stages"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, sensor_depths=sensors, depth_gate=dgate, view_weights=vspec,
                                                                             edge_gate=gate)))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del planes, agg
        del sensors, probs
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def kernel_run(name):
    g = next(x for x in GEOMETRIES if x["name"] == name)
    mesh = synth.grid_mesh(1000, 500)
    r = render.triangles(mesh)
    cams, sensors, probs = setup(g, r, np.float32)
    agg = fusion.MeshAggregator(len(mesh.faces), g["classes"])
    for radius in RADII:
        gate = fusion.EdgeGate(radius, **GATE)
        for _ in range(5):
            agg.fuse_views(r, cams, probs, edge_gate=gate)
        _lib.synchronize(0)
    for _ in range(5):      # the yardstick of the same session: k_depth_weights on full-size float32 sensor planes
        agg.fuse_views(r, cams, probs, sensor_depths=sensors, depth_gate=fusion.DepthGate(0.05))
    _lib.synchronize(0)


def merge(csv_path, name, out_path):
    """The kernel trace holds k_edge_weights' launches of both radii under one name: they are split by their order in time, ten
    launches (five calls of two groups) per radius."""
    g = next(x for x in GEOMETRIES if x["name"] == name)
    W, H = g["target"]
    table = list(csv.DictReader(open(csv_path)))
    result = json.load(open(out_path))
    entry = {"geometry": name, "views_per_launch": 8, "source": "rocprofv3 --kernel-trace, a run of its own (5 calls of leg a per radius, 5 depth-gated calls)"}
    if table and "Start_Timestamp" in table[0]:
        rows = sorted((row for row in table if "k_edge_weights" in row.get("Kernel_Name", "")), key=lambda row: int(row["Start_Timestamp"]))
        per = len(rows) // len(RADII)
        groups = [("k_edge_weights_radius_%d" % radius, rows[i * per:(i + 1) * per], 8.0) for i, radius in enumerate(RADII)]
        groups.append(("k_depth_weights", [row for row in table if "k_depth_weights" in row.get("Kernel_Name", "")], 12.0))
        for key, sel, per_pixel in groups:
            if not sel:
                continue
            us = sorted((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in sel)
            launch_bytes = 8 * W * H * per_pixel
            entry[key] = {"launches": len(us), "median_us_per_launch": statistics.median(us), "min_max_us": [us[0], us[-1]],
                          "us_per_view": statistics.median(us) / 8, "needed_bytes_per_pixel": per_pixel,
                          "share_of_8_TB_per_s": launch_bytes / (statistics.median(us) * 1e-6) / HBM_BYTES_PER_S}
    else:
        raise SystemExit("%s is not a kernel trace (no Start_Timestamp column)" % csv_path)
    result.setdefault("kernel_trace", [])
    result["kernel_trace"] = [e for e in result["kernel_trace"] if e["geometry"] != name] + [entry]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("merged", name, "into", out_path)


FORM_RADII, FORM_CALLS = (1, 2, 8), 20


def form_run():
    mesh = synth.grid_mesh(1000, 500)
    r = render.triangles(mesh)
    depth = r.render(synth.ring_camera(0, VIEWS, 1920, 1080))[1]
    w = fusion.edge_weights_device(depth, fusion.EdgeGate(1, **GATE))
    _lib.synchronize(0)
    for radius in FORM_RADII:
        gate = fusion.EdgeGate(radius, **GATE)
        for _ in range(FORM_CALLS):
            fusion.edge_weights_device(depth, gate, w)
        _lib.synchronize(0)


def merge_form(csv_path, label, out_path):
    table = list(csv.DictReader(open(csv_path)))
    rows = sorted((row for row in table if "k_edge_weights" in row.get("Kernel_Name", "")), key=lambda row: int(row["Start_Timestamp"]))[1:]
    if len(rows) != FORM_CALLS * len(FORM_RADII):
        raise SystemExit("%s holds %d launches of k_edge_weights behind the first, not %d" % (csv_path, len(rows), FORM_CALLS * len(FORM_RADII)))
    out = {"plane": [1920, 1080], "launches_per_radius": FORM_CALLS, "source": "rocprofv3 --kernel-trace of `edge_gate_bench.py form`"}
    for i, radius in enumerate(FORM_RADII):
        us = sorted((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows[i * FORM_CALLS:(i + 1) * FORM_CALLS])
        out["radius_%d" % radius] = {"median_us": statistics.median(us), "min_max_us": [us[0], us[-1]]}
    result = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "tools/edge_gate_bench.py"}
    result.setdefault("form", {})[label] = out
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({label: out}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "kernel":
        kernel_run(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else DEFAULT_OUT)
    elif len(sys.argv) > 1 and sys.argv[1] == "form":
        form_run()
    elif len(sys.argv) > 3 and sys.argv[1] == "merge_form":
        merge_form(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else DEFAULT_OUT)
    else:
        main()
