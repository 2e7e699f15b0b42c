"""fuse_views for cameras with lens distortion (include/smesh_lens.h) at the two geometries the reference's scripts use, on the
1 M-triangle mesh: 16 views per call, medians of 7 repeats with min - max after a warm-up that is not timed; a leg's time is a host
clock around smesh_synchronize for the call, per view.  All legs run in one process.
  scannet      640 x 480 sources -> 1296 x 968, 40 classes
  cityscapes   1024 x 512 sources -> 1920 x 1080, 19 classes
each with a SIMPLE_RADIAL lens (k = -0.12) and an OPENCV lens (k = -0.25, 0.08, p = 0.01, -0.008), f and c those of the view
(synth.ring_camera's), seen through the default view.  The sources are float32 class vectors on the device, (w,h,C) dense.
  a  fuse_views(undistort=True)                                                 (k_undistort_probs per view, then the fusion)
  b  fuse_views on planes and weights undistorted beforehand                    (the floor: what fusing with weights costs)
  c  plain fuse_views(resize="bilinear") on the same sources                    (k_resize_probs: the same bytes, no lens)
  d  host uint8 masks through fuse_views_labels(undistort=True)
  e  the numpy restatement (tests/lens_ref.py) through the host, ONE view
The accumulators of a and b are compared in bits over all views, those of a and e over the first E_VIEWS views (the restatement is
slow); the tool stops if they differ.
`python tools/lens_bench.py kernel <geometry> <lens>` runs k_undistort_probs and k_resize_probs five times each on the same source
and target sizes and nothing else: the run to put under a kernel trace; `python tools/lens_bench.py merge <stats csv> <geometry>
<lens> [output file]` adds both durations and their ratio to the output file.
`python tools/lens_bench.py forms <development libsmesh_hip.so> [output file]` is the one comparison of two forms of
k_undistort_probs' vector path: the tree's library (LDS: a workgroup maps its run of pixels once, one barrier) against a development
build in which every lane recomputes its pixel's map (no LDS, no barrier).  FORMS_ROUNDS alternating rounds, each form in a process
of its own (SMESH_LIB_PATH), 16 launches per repeat, medians of 7 repeats with min - max, at ScanNet's geometry with 40 classes in
float32 (ten lanes a pixel) and float16 (five), the DECIDING cases, and with 8 and 4 float32 classes (two lanes, one lane) beside them.
THE RULE, written before the run: a form is faster in a case when, in every round, its slowest repeat is faster than the other form's
fastest.  The LDS form stays only if it is faster in at least one deciding case and the recompute form is faster in none; in every
other outcome -- a tie included -- the recompute form, the simpler of the two, replaces it.  Exactly one form is kept in the tree.
usage: python tools/lens_bench.py [output file, default profiles/lens_bench.json]"""
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
from semantic_meshes_amd import _lib, data, fusion, render, synth    # noqa: E402
from semantic_meshes_amd.device import to_device                     # noqa: E402
import lens_ref                                                      # noqa: E402

VIEWS, REPS, E_VIEWS, E_REPS = 16, 7, 2, 7
FORMS_ROUNDS = 2
FORM_CASES = ((40, "float32", True), (40, "float16", True), (8, "float32", False), (4, "float32", False))      # classes, dtype, deciding
GEOMETRIES = ({"name": "scannet", "source": (640, 480), "target": (1296, 968), "classes": 40},
              {"name": "cityscapes", "source": (1024, 512), "target": (1920, 1080), "classes": 19})
LENSES = ({"name": "simple_radial", "model": "SIMPLE_RADIAL", "k": (-0.12,), "p": ()},
          {"name": "opencv", "model": "OPENCV", "k": (-0.25, 0.08), "p": (0.01, -0.008)})
DEFAULT_OUT = os.path.join(ROOT, "profiles", "lens_bench.json")


def wall_ms(run, views):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    run()
    _lib.synchronize(0)
    return 1e3 * (time.perf_counter() - t0) / views


def measure(run, warm=2, reps=REPS, views=VIEWS):
    for _ in range(warm):
        run()
    _lib.synchronize(0)
    return [wall_ms(run, views) for _ in range(reps)]


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def lens_cameras(g, ln):
    """(pinhole cameras, LensCameras with the same pose and f, the restated lens and view)."""
    W, H = g["target"]
    cams = [synth.ring_camera(k, VIEWS, W, H) for k in range(VIEWS)]
    lcams = [data.LensCamera(c.rotation, c.translation, np.array([W, H]), c.focal_lengths, c.principal_point, ln["model"],
                             lens_ref.distortion_params(ln["model"], ln["k"], ln["p"])) for c in cams]
    lens = lens_ref.make_lens(ln["model"], cams[0].focal_lengths, cams[0].principal_point, ln["k"], ln["p"], (W, H))
    return cams, lcams, lens, lens_ref.default_view(lens)


def sources(g):
    (w, h), C = g["source"], g["classes"]
    probs = [synth.device_probs(w, h, C, 100 + k) for k in range(VIEWS)]
    rng = np.random.default_rng(5)
    masks = [rng.integers(0, C, size=(w, h)).astype(np.uint8) for _ in range(VIEWS)]
    return probs, masks


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    result = {"tool": "tools/lens_bench.py", "views_per_call": VIEWS, "reps": REPS, "reps_e": E_REPS, "mesh_triangles": P,
              "timing": "host clock around smesh_synchronize for one call of %d views (a - d) or of one view (e), microseconds per view" % VIEWS,
              "cases": []}
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (w, h), (W, H), C = g["source"], g["target"], g["classes"]
        probs, masks = sources(g)
        for ln in LENSES:
            cams, lcams, lens, view = lens_cameras(g, ln)
            case = {"geometry": g["name"], "lens": ln["name"], "source": [w, h], "target": [W, H], "classes": C}

            def leg_e(a, views):
                for k in views:
                    out, inside = lens_ref.ref_undistort_probs(np.asarray(probs[k]), lens, view)
                    a.fuse_views(r, [lcams[k]], [to_device(out)], [to_device(lens_ref.ref_weights(inside))])

            # the legs give the same sums: checked once per case
            a = fusion.MeshAggregator(P, C)
            a.fuse_views(r, lcams, probs, undistort=True)
            case["kernel"] = _lib.last_fuse_kernel()
            planes = [fusion.undistort_probs_device(probs[k], lcams[k], return_weights=True, return_counts=True) for k in range(VIEWS)]
            case["counts_pixels_outside"] = [int(x) for x in sum(p[2] for p in planes)]
            b = fusion.MeshAggregator(P, C)
            b.fuse_views(r, lcams, [p[0] for p in planes], [p[1] for p in planes])
            a2, e = fusion.MeshAggregator(P, C), fusion.MeshAggregator(P, C)
            a2.fuse_views(r, lcams[:E_VIEWS], probs[:E_VIEWS], undistort=True)
            leg_e(e, range(E_VIEWS))
            case["bit_equal_a_b"] = bool(np.array_equal(a.get_raw().view(np.uint32), b.get_raw().view(np.uint32)))
            case["bit_equal_a_e_first_views"] = bool(np.array_equal(a2.get_raw().view(np.uint32), e.get_raw().view(np.uint32)))
            if not (case["bit_equal_a_b"] and case["bit_equal_a_e_first_views"]):
                raise SystemExit("the legs disagree: %s" % json.dumps(case))
            del a, b, a2, e

            agg = fusion.MeshAggregator(P, C)
            case["a"] = stats(measure(lambda: agg.fuse_views(r, lcams, probs, undistort=True)))
            case["b"] = stats(measure(lambda: agg.fuse_views(r, lcams, [p[0] for p in planes], [p[1] for p in planes])))
            case["c"] = stats(measure(lambda: agg.fuse_views(r, cams, probs, resize="bilinear")))
            case["d"] = stats(measure(lambda: agg.fuse_views_labels(r, lcams, masks, undistort=True)))
            case["e"] = stats(measure(lambda: leg_e(agg, [0]), warm=0, reps=E_REPS, views=1))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del planes, agg
        del probs, masks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def kernel_run(gname, lname):
    g = next(x for x in GEOMETRIES if x["name"] == gname)
    ln = next(x for x in LENSES if x["name"] == lname)
    cams, lcams, lens, view = lens_cameras(g, ln)
    probs, _ = sources(g)
    for _ in range(5):
        for k in range(VIEWS):
            fusion.undistort_probs_device(probs[k], lcams[k], return_weights=True)
            fusion.resize_probs_device(probs[k], g["target"])
    _lib.synchronize(0)


def merge(csv_path, gname, lname, out_path):
    rows = list(csv.DictReader(open(csv_path)))

    def avg_us(kernel):
        mine = [row for row in rows if kernel in row.get("Name", "")]
        if not mine:
            raise SystemExit("no %s row in %s" % (kernel, csv_path))
        calls = sum(int(row["Calls"]) for row in mine)
        return sum(float(row["TotalDurationNs"]) for row in mine) / calls / 1e3, calls

    generic = not any("k_undistort_probs<" in row.get("Name", "") for row in rows)      # 19 classes: both kernels' generic forms
    lens_us, lens_calls = avg_us("k_undistort_probs_generic" if generic else "k_undistort_probs<")
    resize_us, resize_calls = avg_us("k_resize_probs_generic" if generic else "k_resize_probs<")

    def std_us(kernel):
        return max(float(row["StdDev"]) for row in rows if kernel in row.get("Name", "")) / 1e3
    result = json.load(open(out_path))
    for case in result["cases"]:
        if case["geometry"] == gname and case["lens"] == lname:
            case["kernels"] = {"k_undistort_probs_us": lens_us, "k_undistort_probs_calls": lens_calls, "k_resize_probs_us": resize_us,
                               "k_resize_probs_calls": resize_calls, "ratio": lens_us / resize_us, "form": "generic" if generic else "vector",
                               "k_undistort_probs_stddev_us": std_us("k_undistort_probs"), "k_resize_probs_stddev_us": std_us("k_resize_probs"),
                               "source": "rocprofv3 --kernel-trace --stats, a run of its own (5 x 16 launches of each kernel)"}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("merged", gname, lname, "into", out_path)


def forms_leg():
    """One form, this process's library: {case: [us per image of each repeat]} as one JSON line."""
    g = GEOMETRIES[0]
    cams, lcams, lens, view = lens_cameras(g, LENSES[0])
    (w, h), out = g["source"], {"path": []}
    for C, dtype, _ in FORM_CASES:
        probs = [synth.device_probs(w, h, C, 100 + k, dtype=dtype) for k in range(VIEWS)]
        run = lambda: [fusion.undistort_probs_device(probs[k], lcams[k], return_weights=True) for k in range(VIEWS)]
        out["%d_%s" % (C, dtype)] = [1e3 * x for x in measure(run)]
        out["path"].append(_lib.get_option("last_lens_path"))
        del probs
    print(json.dumps(out))


def forms(dev_lib, out_path):
    import subprocess
    rounds = []
    for _ in range(FORMS_ROUNDS):
        one = {}
        for form, lib in (("lds", None), ("recompute", dev_lib)):
            env = dict(os.environ)
            env.pop("SMESH_LIB_PATH", None)
            if lib:
                env["SMESH_LIB_PATH"] = os.path.abspath(lib)
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "forms-leg"], env=env, check=True, capture_output=True, text=True).stdout
            one[form] = json.loads(text.strip().split("\n")[-1])
            if any(p != 1 for p in one[form].pop("path")):
                raise SystemExit("a case of the %s form did not take the vector path" % form)
        rounds.append(one)
    cases, lds_wins, rec_wins = {}, 0, 0
    for C, dtype, deciding in FORM_CASES:
        key = "%d_%s" % (C, dtype)
        lds_faster = all(max(r["lds"][key]) < min(r["recompute"][key]) for r in rounds)
        rec_faster = all(max(r["recompute"][key]) < min(r["lds"][key]) for r in rounds)
        cases[key] = {"deciding": deciding, "faster": "lds" if lds_faster else "recompute" if rec_faster else "tie",
                      "rounds": [{f: {"median_us": statistics.median(r[f][key]), "min_max_us": [min(r[f][key]), max(r[f][key])]} for f in r} for r in rounds]}
        lds_wins += deciding and lds_faster
        rec_wins += deciding and rec_faster
    keep = "lds" if (lds_wins >= 1 and rec_wins == 0) else "recompute"
    result = json.load(open(out_path)) if os.path.exists(out_path) else {}
    result["forms"] = {"rule": "a form is faster in a case when in every round its slowest repeat beats the other's fastest; the LDS form stays "
                               "only if faster in at least one deciding case and the recompute form in none, else the recompute form (the simpler)",
                       "geometry": "scannet", "lens": LENSES[0]["name"], "launches_per_repeat": VIEWS, "reps": REPS, "rounds": FORMS_ROUNDS,
                       "timing": "host clock around smesh_synchronize for %d undistort_probs_device calls, microseconds per image" % VIEWS,
                       "cases": cases, "kept": keep}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["forms"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "forms-leg":
        forms_leg()
    elif len(sys.argv) > 2 and sys.argv[1] == "forms":
        forms(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT)
    elif len(sys.argv) > 3 and sys.argv[1] == "kernel":
        kernel_run(sys.argv[2], sys.argv[3])
    elif len(sys.argv) > 4 and sys.argv[1] == "merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] if len(sys.argv) > 5 else DEFAULT_OUT)
    else:
        main()
