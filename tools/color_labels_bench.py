"""fuse_views_labels on COLOUR masks (include/smesh_label_colors.h) on the 1 M-triangle mesh, by the method of
tools/label_prepare_bench.py: 16 masks per call, medians of 7 repeats with min - max after a warm-up that is not timed; a leg's time is
a host clock around smesh_synchronize for the call, in microseconds per view.  All legs run in one process, one after the other per
case.  The device masks are decoded (h,w,3) images passed as their transposed (w,h,3) views.
  cityscapes       1024 x 512 -> 1920 x 1080, 19 colours        cityscapes-full  1920 x 1080, no resize, 19 colours
  scannet          640 x 480 -> 1296 x 968, 40 colours
each with masks of uniform regions (32 x 32-pixel blocks of one colour) and with random ones (every pixel drawn by itself: the worst
case for the bitmap's "bit already set" test and for the lookup's locality).
  a  palette= with a known table                                             (k_labels_prepare_colors)
  b  palette=ColorRemap(): a fresh remap per call, so every call discovers   (k_colors_mark / _count / _list, then a)
  c  full-size planes prepared beforehand                                    (the floor: no preparation at all)
  d  what the library offered before: keys packed with numpy into a uint32 image per call, then label_map= with a 2^24-entry table
     (kept on the device, which flatters this leg: a host table would cross PCIe, 64 MB, on every call)
  e  the script's own host route for ONE image: np.unique(axis=0, return_inverse=True), the dictionary, numpy index upsampling where
     the sizes differ, and the plain call; 3 repeats
  f  host (numpy) masks with palette=
  g  table sizes 19 (or 40), 1 358 and lds_max + 904 with palette= (the extra entries are colours no mask holds)
The accumulators of a, b, c and d are compared in bits once per case.

RULE, stated before the run: the neighbour-key shortcut (a lane dropping a key equal to its neighbour's before the bitmap test of
k_colors_mark, or reusing its neighbour's lookup in k_labels_prepare_colors) stays only where it is faster beyond the min - max
spread of both legs on the uniform masks and not slower beyond it on the random ones; otherwise the simpler form stays.
What it decided (the "mark_forms" section of the JSON, measured with a temporary option that chose the form per call in this
process and was removed afterwards): in k_colors_mark the compare with the left neighbour lane passed on all three geometries and
is the only form now; a wave-wide form (one lane per distinct key of a wave) lost on random masks and is gone; the lookup has no
shortcut and was not measured with one.

usage: python tools/color_labels_bench.py [output file, default profiles/color_labels_bench.json]
       (an existing output file's "mark_forms", "kernels" and "unchanged_paths" sections are kept)
       python tools/color_labels_bench.py --profile-run             legs a and b of cityscapes / uniform only, for a kernel trace
       python tools/color_labels_bench.py --kernel-stats STATS.csv [output file]     merge a kernel trace's statistics into the file
       python tools/color_labels_bench.py --unchanged LABEL NAME=JSONFILE ... [output file]     merge runs of the unchanged paths"""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES, REPS = 16, 7
DEFAULT_OUT = os.path.join(ROOT, "profiles", "color_labels_bench.json")
GEOMETRIES = ({"name": "cityscapes", "source": (1024, 512), "target": (1920, 1080), "colours": 19},
              {"name": "cityscapes-full", "source": (1920, 1080), "target": (1920, 1080), "colours": 19},
              {"name": "scannet", "source": (640, 480), "target": (1296, 968), "colours": 40})
HBM_BYTES_PER_S = 8e12


def stats(samples):
    return {"median_us": 1e3 * statistics.median(samples), "min_max_us": [1e3 * min(samples), 1e3 * max(samples)]}


def axis_index(n, N):
    return ((2 * np.arange(N, dtype=np.int64) + 1) * n) // (2 * N)


def make_masks(rng, w, h, palette, uniform):
    """IMAGES decoded (h,w,3) images and their class images (h,w)."""
    K = len(palette)
    out = []
    for _ in range(IMAGES):
        if uniform:
            coarse = rng.integers(0, K, size=(h // 32 + 1, w // 32 + 1))
            cls = np.repeat(np.repeat(coarse, 32, axis=0), 32, axis=1)[:h, :w]
            cls[0, :K] = np.arange(K)[:w]          # every colour in every mask: the remap numbers them like the known table
        else:
            cls = rng.integers(0, K, size=(h, w))
        out.append(np.ascontiguousarray(palette[cls]))
    return out


def bench(out_path, profile_run=False):
    from semantic_meshes_amd import _lib, fusion, render, synth
    from semantic_meshes_amd.device import to_device

    def wall_ms(run, views):
        _lib.synchronize(0)
        t0 = time.perf_counter()
        run()
        _lib.synchronize(0)
        return 1e3 * (time.perf_counter() - t0) / views

    def measure(run, warm=2, reps=REPS, views=IMAGES):
        for _ in range(warm):
            run()
        _lib.synchronize(0)
        return stats([wall_ms(run, views) for _ in range(reps)])

    lds_max = _lib.get_option("labels_colors_lds_max")
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    result = {"tool": "tools/color_labels_bench.py", "images_per_call": IMAGES, "reps": REPS, "mesh_triangles": P, "labels_colors_lds_max": lds_max,
              "timing": "host clock around smesh_synchronize for one call of %d masks, microseconds per view" % IMAGES,
              "neighbour_key_shortcut": "k_colors_mark: the left-neighbour compare, kept by the rule in the tool's docstring (mark_forms); k_labels_prepare_colors: none", "cases": []}
    r = render.triangles(mesh)
    for g in GEOMETRIES[:1] if profile_run else GEOMETRIES:
        for uniform in (True,) if profile_run else (True, False):
            (w, h), (W, H), K = g["source"], g["target"], g["colours"]
            C = K
            rng = np.random.default_rng(11)
            keys = rng.permutation(np.unique(rng.integers(0, 1 << 24, size=3 * (K + lds_max + 904))))[:K + lds_max + 904]
            colours = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=-1).astype(np.uint8)
            palette = colours[:K][np.argsort(keys[:K])]          # class = rank of the key: what a remap of a mask with every colour gives
            cams = [synth.ring_camera(k, IMAGES, W, H) for k in range(IMAGES)]
            decoded = make_masks(rng, w, h, palette, uniform)
            host = [x.transpose(1, 0, 2) for x in decoded]
            dev = [to_device(x).transpose(1, 0, 2) for x in decoded]
            resize = None if (w, h) == (W, H) else "nearest"
            table = fusion.ColorTable(palette)
            case = {"geometry": g["name"], "masks": "uniform" if uniform else "random", "source": [w, h], "target": [W, H], "colours": K, "classes": C}
            agg = fusion.MeshAggregator(P, C)
            leg_a = lambda: agg.fuse_views_labels(r, cams, dev, resize=resize, palette=table)                    # noqa: E731
            leg_b = lambda: agg.fuse_views_labels(r, cams, dev, resize=resize, palette=fusion.ColorRemap())      # noqa: E731
            if profile_run:
                for _ in range(3):
                    leg_a()
                    leg_b()
                _lib.synchronize(0)
                print("profile run done: %s" % json.dumps(case))
                return
            full = [fusion.prepare_labels_device(x, C, (W, H), resize, palette=table) for x in dev]
            big_map = np.full(1 << 24, -1, np.int32)
            big_map[table.keys] = table.classes
            big_map = to_device(big_map)

            def packed():
                return [(x[..., 0].astype(np.uint32) << 16) | (x[..., 1].astype(np.uint32) << 8) | x[..., 2] for x in host]

            leg_c = lambda: agg.fuse_views_labels(r, cams, full)                                                 # noqa: E731
            leg_d = lambda: agg.fuse_views_labels(r, cams, packed(), resize=resize, label_map=big_map)           # noqa: E731
            # the legs give the same sums: checked once per case
            sums = []
            for leg in (leg_a, leg_b, leg_c, leg_d):
                agg = fusion.MeshAggregator(P, C)
                leg()
                sums.append(agg.get_raw().view(np.uint32))
            case["bit_equal_a_b_c_d"] = bool(all(np.array_equal(sums[0], s) for s in sums[1:]) and sums[0].any())
            del sums
            agg = fusion.MeshAggregator(P, C)
            case["a"], case["b"], case["c"] = measure(leg_a), measure(leg_b), measure(leg_c)
            case["d"] = measure(leg_d, warm=1)

            def script_route():
                mask = decoded[0].reshape(-1, 3)
                uniq, inv = np.unique(mask, axis=0, return_inverse=True)
                d = {}
                cls = np.array([d.setdefault(tuple(c.tolist()), len(d)) for c in uniq])
                m = cls[inv.reshape(-1)].reshape(h, w).T
                if resize:
                    m = m[axis_index(w, W)[:, None], axis_index(h, H)[None, :]]
                agg.fuse_views_labels(r, cams[:1], [m])

            case["e"] = measure(script_route, warm=0, reps=3, views=1)
            case["f"] = measure(lambda: agg.fuse_views_labels(r, cams, host, resize=resize, palette=table), warm=1)
            case["g"] = {}
            for extra in (0, 1358 - K, lds_max + 904 - K):
                t = fusion.ColorTable(np.concatenate([palette, colours[K:K + extra]]), np.concatenate([np.arange(K), np.full(extra, -1)]))
                case["g"]["%d entries" % len(t)] = measure(lambda: agg.fuse_views_labels(r, cams, dev, resize=resize, palette=t))
            case["needed_bytes_per_view"] = {"k_colors_mark": 3 * w * h + (1 << 21), "k_labels_prepare_colors": 3 * w * h + W * H}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del dev, full, agg, big_map
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    if os.path.exists(out_path):
        with open(out_path) as f:
            old = json.load(f)
        result.update({k: old[k] for k in ("mark_forms", "kernels", "unchanged_paths") if k in old})
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def merge_kernel_stats(stats_csv, out_path):
    """The colour kernels' rows of a `rocprofv3 --kernel-trace --stats` run of `--profile-run` (cityscapes, uniform masks), with the
    bytes each launch needs as a share of 8 TB/s."""
    with open(out_path) as f:
        result = json.load(f)
    (w, h), (W, H) = GEOMETRIES[0]["source"], GEOMETRIES[0]["target"]
    need = {"k_colors_mark": 3 * w * h + (1 << 21), "k_labels_prepare_colors": 3 * w * h + W * H,
            "k_colors_count": 8 * (1 << 21), "k_colors_list": 8 * (1 << 21)}
    rows = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for name, nbytes in need.items():
                if name in row["Name"]:
                    avg = float(row["AverageNs"])
                    rows[row["Name"]] = {"calls": int(row["Calls"]), "average_us": avg / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                         "max_us": float(row["MaxNs"]) / 1e3, "needed_bytes": nbytes,
                                         "share_of_8_TB_per_s": nbytes / (avg * 1e-9) / HBM_BYTES_PER_S}
    result["kernels"] = {"run": "rocprofv3 --kernel-trace --stats -- python tools/color_labels_bench.py --profile-run (a run of its own: "
                                "cityscapes 1024 x 512 -> 1920 x 1080, uniform masks; k_colors_count / _list serve eight bitmaps a launch)",
                         "rows": rows}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("merged %d kernel rows into %s" % (len(rows), out_path))


def merge_unchanged(args, out_path):
    """`--unchanged LABEL NAME=FILE ...`: results of the unchanged paths (bench.py's JSON line, leg a of label_prepare_bench.py) measured
    in the same session on the parent commit's library and on this one's, copied into the file under unchanged_paths[LABEL][NAME]."""
    with open(out_path) as f:
        result = json.load(f)
    label, pairs = args[0], args[1:]
    for pair in pairs:
        name, path = pair.split("=", 1)
        with open(path) as f:
            text = f.read().strip()
        try:
            value = json.loads(text)
        except ValueError:
            value = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
        if isinstance(value, dict) and "cases" in value:      # label_prepare_bench.py: leg a of each case
            value = {c["geometry"]: c["a"] for c in value["cases"]}
        result.setdefault("unchanged_paths", {}).setdefault(label, {})[name] = value
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("merged %s into %s" % (label, out_path))


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--profile-run":
        bench(None, profile_run=True)
    elif argv and argv[0] == "--kernel-stats":
        merge_kernel_stats(argv[1], argv[2] if len(argv) > 2 else DEFAULT_OUT)
    elif argv and argv[0] == "--unchanged":
        rest = argv[1:]
        out = rest.pop() if rest and "=" not in rest[-1] and len(rest) > 1 and rest[-1].endswith(".json") else DEFAULT_OUT
        merge_unchanged(rest, out)
    else:
        bench(argv[0] if argv else DEFAULT_OUT)
