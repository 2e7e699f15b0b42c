"""fuse_views on class-vector images at the network's resolution: resample-then-fuse (`resize="bilinear"`) against sampling inside the
fusion kernel (`sample_in_kernel=True`, include/smesh_sampled.h), at the two geometries the reference's scripts use -- 640 x 480 ->
1296 x 968 with 40 classes (ScanNet) and 1024 x 512 -> 1920 x 1080 with 19 (Cityscapes) -- on the 1 M-triangle mesh, in float32,
float16 and bfloat16.  16 device-resident images per call, medians of 7 repeats with min - max, a warm-up that is not timed; a leg's
time is a host clock around smesh_synchronize for the call, per view.  All legs run in one process:
  i    fuse_views(..., resize="bilinear")                               (the existing route)
  ii   fuse_views(..., resize="bilinear", sample_in_kernel=True)        (k_fuse_tri_sampled)
  iii  fuse_views on images resampled beforehand                         (the floor: no resampling at all)
  iv   ii with host images against i with host images
Beside them: the fusion kernels' own time per view in i, ii and iii (the library's HIP-event profile slot, in runs of their own), and
the device memory the call made the library map (hipMemGetInfo before the call, after a trim of the library's block cache, against
after it).  The cache keeps every block the call freed, so the figure includes them: it is an upper bound on what was alive at once.
Route i works in chunks of eight views and the figure is all 16 resampled images, so between half of it and all of it was alive.
"ii_faster_beyond_spread": the median of ii is below the median of i by more than both legs' min - max spreads.
usage: python tools/sampled_fuse_bench.py [output file, default profiles/sampled_fuse_bench.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, fusion, render, synth          # noqa: E402

IMAGES, REPS = 16, 7
GEOMETRIES = ({"name": "scannet", "source": (640, 480), "target": (1296, 968), "classes": 40},
              {"name": "cityscapes", "source": (1024, 512), "target": (1920, 1080), "classes": 19})
DTYPES = ("float32", "float16", "bfloat16")
SAMPLED = {"resize": "bilinear", "sample_in_kernel": True}


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


def fuse_kernel_us(run):
    """Microseconds per view that the fusion kernels of `run()` took: the library's HIP-event slot, median of REPS runs of their own."""
    lib = _lib.lib()
    out = []
    for _ in range(REPS):
        _lib.check(lib.smesh_profile_sample_every(0, 1))
        _lib.check(lib.smesh_profile_reset(0))
        _lib.check(lib.smesh_profile_enable(0, 1 << _lib.PROF_FUSE_SCATTER))
        run()
        _lib.synchronize(0)
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        _lib.check(lib.smesh_profile_read(0, _lib.PROF_FUSE_SCATTER, ctypes.byref(ms), ctypes.byref(n)))
        _lib.check(lib.smesh_profile_enable(0, 0))
        out.append(1e3 * ms.value / IMAGES)
    return statistics.median(out)


def free_bytes():
    hip = ctypes.CDLL(None)                    # the HIP runtime the library runs on is in the process already
    if not hasattr(hip, "hipMemGetInfo"):
        hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise SystemExit("hipMemGetInfo failed")
    return free.value


def held_bytes(run):
    """Device memory `run()` made the library map: the block cache is emptied first and keeps what the call frees, so blocks freed
    during the call count too -- an upper bound on the bytes alive at once."""
    _lib.synchronize(0)
    _lib.check(_lib.lib().smesh_device_trim(0, None))
    before = free_bytes()
    run()
    _lib.synchronize(0)
    return max(before - free_bytes(), 0)


def spread(s):
    return s["min_max_us"][1] - s["min_max_us"][0]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sampled_fuse_bench.json")
    result = {"tool": "tools/sampled_fuse_bench.py", "images_per_call": IMAGES, "reps": REPS, "mesh_triangles": None,
              "timing": "host clock around smesh_synchronize for one fuse_views call of %d device-resident images, per view" % IMAGES,
              "cases": []}
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    result["mesh_triangles"] = P
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (w, h), (W, H), C = g["source"], g["target"], g["classes"]
        cams = [synth.ring_camera(k, IMAGES, W, H) for k in range(IMAGES)]
        for dtype in DTYPES:
            kw = {"probs_dtype": "bfloat16"} if dtype == "bfloat16" else {}
            small = [synth.device_probs(w, h, C, 1000 + k, dtype=dtype) for k in range(IMAGES)]
            agg = fusion.MeshAggregator(P, C)
            case = {"geometry": g["name"], "source": [w, h], "target": [W, H], "classes": C, "dtype": dtype}

            def leg_i():
                agg.fuse_views(r, cams, small, resize="bilinear", **kw)

            def leg_ii():
                agg.fuse_views(r, cams, small, **SAMPLED, **kw)

            # the two routes give the same sums: checked once per case on what the warm-up calls left
            a, b = fusion.MeshAggregator(P, C), fusion.MeshAggregator(P, C)
            a.fuse_views(r, cams, small, resize="bilinear", **kw)
            b.fuse_views(r, cams, small, **SAMPLED, **kw)
            if _lib.last_fuse_kernel() != "k_fuse_tri_sampled":
                raise SystemExit("leg ii did not take k_fuse_tri_sampled (%s, %s)" % (g["name"], dtype))
            ra, rb = a.get_raw(), b.get_raw()
            case["max_relative_difference_i_ii"] = float(np.max(np.abs(ra - rb) / np.maximum(np.abs(ra), 1e-30)))
            case["bit_equal_i_ii"] = bool(np.array_equal(ra.view(np.uint32), rb.view(np.uint32)))
            del a, b, ra, rb

            case["held_bytes_i"] = held_bytes(leg_i)
            case["held_bytes_ii"] = held_bytes(leg_ii)
            case["i"] = stats(measure(leg_i))
            case["ii"] = stats(measure(leg_ii))
            case["fusion_kernel_us_per_view_i"] = fuse_kernel_us(leg_i)
            case["fusion_kernel_us_per_view_ii"] = fuse_kernel_us(leg_ii)
            full = [fusion.resize_probs_device(s, (W, H), **kw) for s in small]
            case["iii"] = stats(measure(lambda: agg.fuse_views(r, cams, full, **kw)))
            case["fusion_kernel_us_per_view_iii"] = fuse_kernel_us(lambda: agg.fuse_views(r, cams, full, **kw))
            del full
            host = [np.asarray(s) for s in small]
            case["iv"] = {"i_host": stats(measure(lambda: agg.fuse_views(r, cams, host, resize="bilinear", **kw), warm=1)),
                          "ii_host": stats(measure(lambda: agg.fuse_views(r, cams, host, **SAMPLED, **kw), warm=1))}
            d = case["i"]["median_us"] - case["ii"]["median_us"]
            case["ii_minus_i_us"] = -d
            case["ii_faster_beyond_spread"] = bool(d > max(spread(case["i"]), spread(case["ii"])))
            case["ii_slower_beyond_spread"] = bool(-d > max(spread(case["i"]), spread(case["ii"])))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del small, host, agg
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
