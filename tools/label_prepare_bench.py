"""fuse_views_labels on masks at the network's resolution and in the dataset's ids (include/smesh_label_prep.h), at the two geometries
the reference's scripts use, on the 1 M-triangle mesh: 16 masks per call, medians of 7 repeats with min - max after a warm-up that is
not timed; a leg's time is a host clock around smesh_synchronize for the call, per view.  All legs run in one process.
  scannet     640 x 480 -> 1296 x 968, 40 classes, uint16 raw ids through a 1 358-entry map
  cityscapes  1024 x 512 -> 1920 x 1080, 19 classes, uint8, no map
The device masks are decoded (h,w) images passed as their transposed (w,h) views, as README.md says to hand a mask over.
  a  fuse_views_labels(resize="nearest", label_map=)                        (k_labels_prepare)
  c  full-size masks prepared beforehand                                    (the floor: no preparation at all)
  d  the route before this entry point: numpy gather and numpy index upsampling on the host, then fuse_views_labels on host masks
  e  full-size transposed int32 device masks: fuse_views_labels without keywords (k_labels_narrow) against prepare_labels_device of
     each mask followed by fuse_views_labels on the planes
  f  host (numpy) masks: small with the keywords against full size without
profiles/label_prepare_bench.json was written when the kernel still had a second, tiled form (leg a, with leg b the form kept here,
chosen by an option "labels_prepare_tiles").  The decision rule, stated before that run: the tiled form stays only if a beats b, or
e's right side beats its left, by more than the min - max spread of both legs.  It did neither, so it was removed with its option
and there is no leg b any more.
usage: python tools/label_prepare_bench.py [output file, default profiles/label_prepare_bench.json]"""
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

IMAGES, REPS = 16, 7
GEOMETRIES = ({"name": "scannet", "source": (640, 480), "target": (1296, 968), "classes": 40, "dtype": "uint16", "map": 1358},
              {"name": "cityscapes", "source": (1024, 512), "target": (1920, 1080), "classes": 19, "dtype": "uint8", "map": 0})


def wall_ms(run):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    run()
    _lib.synchronize(0)
    return 1e3 * (time.perf_counter() - t0) / IMAGES


def measure(run, warm=2):
    for _ in range(warm):
        run()
    _lib.synchronize(0)
    return [wall_ms(run) for _ in range(REPS)]


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def spread(s):
    return s["min_max_us"][1] - s["min_max_us"][0]


def beats(x, y):
    """x is faster than y by more than both legs' min - max spreads."""
    return bool(y["median_us"] - x["median_us"] > max(spread(x), spread(y)))


def axis_index(n, N):
    return ((2 * np.arange(N, dtype=np.int64) + 1) * n) // (2 * N)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "label_prepare_bench.json")
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    result = {"tool": "tools/label_prepare_bench.py", "images_per_call": IMAGES, "reps": REPS, "mesh_triangles": P,
              "timing": "host clock around smesh_synchronize for one call of %d masks, microseconds per view" % IMAGES, "cases": []}
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (w, h), (W, H), C, dt = g["source"], g["target"], g["classes"], np.dtype(g["dtype"])
        rng = np.random.default_rng(11)
        cams = [synth.ring_camera(k, IMAGES, W, H) for k in range(IMAGES)]
        m = None
        if g["map"]:
            m = rng.integers(-1, C, size=g["map"]).astype(np.int32)        # raw id -> class, -1 for "unmapped"
        top = g["map"] or C + 1
        decoded = [rng.integers(0, top, size=(h, w)).astype(dt) for _ in range(IMAGES)]       # (h,w): as an image decoder leaves them
        host = [x.T for x in decoded]                                                         # the (w,h) views
        dev = [to_device(x).T for x in decoded]
        kw = {"resize": "nearest", "label_map": m}
        agg = fusion.MeshAggregator(P, C)
        case = {"geometry": g["name"], "source": [w, h], "target": [W, H], "classes": C, "dtype": dt.name, "map_entries": g["map"]}

        def upsampled(x):
            v = x[axis_index(w, W)[:, None], axis_index(h, H)[None, :]]
            return v if m is None else m[v]

        # the legs give the same sums: checked once per case
        ref_planes = [fusion.narrow_labels(upsampled(x), C) for x in host]
        sums = []
        before = _lib.get_option("labels_prepare_launches")
        a = fusion.MeshAggregator(P, C)
        a.fuse_views_labels(r, cams, dev, **kw)
        sums.append(a.get_raw().view(np.uint32))
        if _lib.get_option("labels_prepare_launches") - before != IMAGES:
            raise SystemExit("leg a did not launch k_labels_prepare once per view (%s)" % g["name"])
        a = fusion.MeshAggregator(P, C)
        a.fuse_views_labels(r, cams, [to_device(p) for p in ref_planes])
        sums.append(a.get_raw().view(np.uint32))
        case["bit_equal_a_c"] = bool(np.array_equal(sums[0], sums[1]))
        del a, sums

        case["a"] = stats(measure(lambda: agg.fuse_views_labels(r, cams, dev, **kw)))
        full = [fusion.prepare_labels_device(x, C, (W, H), **kw) for x in dev]
        case["c"] = stats(measure(lambda: agg.fuse_views_labels(r, cams, full)))
        case["d"] = stats(measure(lambda: agg.fuse_views_labels(r, cams, [upsampled(x) for x in host]), warm=1))
        wide = [to_device(np.ascontiguousarray(np.asarray(p).T.astype(np.int32))).T for p in ref_planes]      # full-size (H,W) int32, transposed views
        case["e"] = {"k_labels_narrow": stats(measure(lambda: agg.fuse_views_labels(r, cams, wide))),
                     "prepare_labels_device_then_fuse": stats(measure(lambda: agg.fuse_views_labels(r, cams, [fusion.prepare_labels_device(x, C) for x in wide])))}
        full_host = [np.ascontiguousarray(upsampled(x)) for x in host]
        case["f"] = {"small_with_keywords": stats(measure(lambda: agg.fuse_views_labels(r, cams, host, **kw), warm=1)),
                     "full_size_plain": stats(measure(lambda: agg.fuse_views_labels(r, cams, full_host), warm=1))}
        case["e_right_beats_left"] = beats(case["e"]["prepare_labels_device_then_fuse"], case["e"]["k_labels_narrow"])
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del dev, full, wide, agg
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
