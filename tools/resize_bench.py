"""Class-vector images resampled from the network's resolution to the camera's (include/smesh_resize.h, fusion.resize_probs_device and
the `resize=` keywords) at the two geometries the reference's scripts use -- 640 x 480 -> 1296 x 968 with 40 classes (ScanNet) and
1024 x 512 -> 1920 x 1080 with 19 (Cityscapes) -- in float32, float16 and bfloat16.  16 device-resident images per leg, medians of 7
repeats with min - max.  These entry points have no profile slot: a leg's time is a host clock around smesh_synchronize for the batch
of 16, per image.

Legs:
  a  smesh_resize_probs into preallocated outputs: microseconds per image, the needed bytes (source once plus output once) against
     8 TB/s; "a_call": fusion.resize_probs_device (the same plus the output's allocation); "a_generic": a with the option
     "resize_vector" at 0
  b  fuse_views(..., resize="bilinear") on the source images against fuse_views on the same images resampled beforehand: the added
     time per view, also as a fraction of the fusion kernels' time (the library's HIP-event profile slot, in a run of its own)
  c  host images: source-size numpy images with resize= against full-size numpy images
  d  the route without this interface, where torch imports and sees the device: torch.nn.functional.interpolate + permute, then
     fuse_views; the whole call, and the largest absolute difference of its image from a's
  e  add_probs(..., resize="bilinear") against resize_probs_device + add_probs; the matrices are checked equal
With --kernel-stats FILE (the kernel statistics CSV of a separate `rocprofv3 --kernel-trace --stats` run of `--trace-leg`) the
average kernel times of k_resize_probs and of k_widen_probs16 -- the project's existing write-dominated streaming kernel, on an image
of the output's size -- are recorded beside leg a.
usage: python tools/resize_bench.py [--trace-leg] [--kernel-stats FILE] [output file, default profiles/resize_bench.json]"""
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, device, fusion, render, synth          # noqa: E402

IMAGES, REPS, PEAK = 16, 7, 8.0e12
GEOMETRIES = ({"name": "scannet", "source": (640, 480), "target": (1296, 968), "classes": 40},
              {"name": "cityscapes", "source": (1024, 512), "target": (1920, 1080), "classes": 19})
DTYPES = ("float32", "float16", "bfloat16")
CODES = {"float32": _lib.PROBS_F32, "float16": _lib.PROBS_F16, "bfloat16": _lib.PROBS_BF16}
ITEM = {"float32": 4, "float16": 2, "bfloat16": 2}


def wall_ms(run):
    """Milliseconds per image of `run()` over the IMAGES images: a host clock around a synchronise."""
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


def fuse_kernel_ms(run):
    """Milliseconds per image that the fusion kernels of `run()` took: the library's HIP-event slot, in a run of its own."""
    lib = _lib.lib()
    _lib.check(lib.smesh_profile_sample_every(0, 1))
    _lib.check(lib.smesh_profile_reset(0))
    _lib.check(lib.smesh_profile_enable(0, 1 << _lib.PROF_FUSE_SCATTER))
    run()
    _lib.synchronize(0)
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.check(lib.smesh_profile_read(0, _lib.PROF_FUSE_SCATTER, ctypes.byref(ms), ctypes.byref(n)))
    _lib.check(lib.smesh_profile_enable(0, 0))
    return ms.value / IMAGES


def torch_or_none():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except Exception:
        return None


def kw_of(dtype):
    return {"probs_dtype": "bfloat16"} if dtype == "bfloat16" else {}


def resize_into(src, out, dtype, size):
    (w, h, C), (W, H) = src.shape, size
    _lib.check(_lib.lib().smesh_resize_probs(ctypes.c_void_p(src.ptr), CODES[dtype], None, _lib.MEM_DEVICE, w, h, C,
                                             ctypes.c_void_p(out.ptr), CODES[dtype], W, H, _lib.RESIZE_BILINEAR, 0))


def kernel_stats(path):
    """{kernel family: average ns} from a rocprofv3 kernel statistics CSV, weighted over the instances of a family."""
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for fam in ("k_resize_probs_labels", "k_resize_probs_generic", "k_resize_probs", "k_widen_probs16"):
                if fam + "<" in row["Name"] or fam + "(" in row["Name"]:
                    t = tot.setdefault(fam, [0, 0])
                    t[0] += int(row["Calls"])
                    t[1] += int(row["TotalDurationNs"])
                    break
    return {fam: {"calls": c, "average_us": 1e-3 * ns / c} for fam, (c, ns) in tot.items() if c}


def trace_leg():
    """What the separate rocprofv3 run executes: float16 images of the ScanNet geometry resampled (k_resize_probs), and the same
    number of float16 images of the OUTPUT's size widened to float32 (k_widen_probs16: a Mul aggregator takes the widening route)."""
    g = GEOMETRIES[0]
    (w, h), (W, H), C = g["source"], g["target"], g["classes"]
    mesh = synth.grid_mesh(200, 100)
    cams = [synth.ring_camera(k, IMAGES, W, H) for k in range(IMAGES)]
    r = render.triangles(mesh)
    small = [synth.device_probs(w, h, C, 100 + k, dtype="float16") for k in range(IMAGES)]
    big = [fusion.resize_probs_device(s, (W, H)) for s in small]
    agg = fusion.MeshAggregator(len(mesh.faces), C, "mul")
    agg.fuse_views(r, cams, big)
    _lib.synchronize(0)


def main():
    args = [a for a in sys.argv[1:]]
    if "--trace-leg" in args:
        trace_leg()
        return
    stats_path = None
    if "--kernel-stats" in args:
        k = args.index("--kernel-stats")
        stats_path = args[k + 1]
        del args[k:k + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "resize_bench.json")
    torch = torch_or_none()
    result = {"tool": "tools/resize_bench.py", "images_per_leg": IMAGES, "reps": REPS, "roofline_bytes_per_s": PEAK,
              "timing": "host clock around smesh_synchronize for a batch of %d device-resident images, per image" % IMAGES,
              "torch_route": "measured" if torch is not None else "not measured", "cases": []}
    if stats_path and os.path.exists(stats_path):
        result["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (tools/resize_bench.py --trace-leg): float16, "
                                            "640x480 -> 1296x968, 40 classes; k_widen_probs16 on float16 images of the output's size",
                                  "kernels": kernel_stats(stats_path)}
        (w, h), (W, H), C = GEOMETRIES[0]["source"], GEOMETRIES[0]["target"], GEOMETRIES[0]["classes"]
        need = {"k_resize_probs": (w * h + W * H) * C * 2, "k_widen_probs16": W * H * C * (2 + 4)}
        for fam, nbytes in need.items():
            k = result["kernel_trace"]["kernels"].get(fam)
            if k:
                k["needed_bytes"] = nbytes
                k["share_of_roofline"] = nbytes / PEAK / (1e-6 * k["average_us"])
    mesh = synth.grid_mesh(1000, 500)          # cfg2's mesh: a million triangles
    P = len(mesh.faces)
    r = render.triangles(mesh)
    for g in GEOMETRIES:
        (w, h), (W, H), C = g["source"], g["target"], g["classes"]
        cams = [synth.ring_camera(k, IMAGES, W, H) for k in range(IMAGES)]
        gt = device.to_device(np.random.default_rng(C).integers(0, C, size=(W, H), dtype=np.uint8))
        for dtype in DTYPES:
            kw = kw_of(dtype)
            small = [synth.device_probs(w, h, C, 1000 + k, dtype=dtype) for k in range(IMAGES)]
            outs = [device.DeviceBuffer(W * H * C * ITEM[dtype]).view((W, H, C), small[0].dtype) for _ in range(IMAGES)]
            for o in outs:
                o.bfloat16 = dtype == "bfloat16"
            need = (w * h + W * H) * C * ITEM[dtype]
            case = {"geometry": g["name"], "source": [w, h], "target": [W, H], "classes": C, "dtype": dtype, "needed_bytes": need}

            def leg_a():
                for s, o in zip(small, outs):
                    resize_into(s, o, dtype, (W, H))
            a = measure(leg_a)
            case["a"] = stats(a)
            case["a"]["share_of_roofline"] = need / PEAK / (1e-3 * statistics.median(a))
            _lib.set_option("resize_vector", 0)
            try:
                case["a_generic"] = stats(measure(leg_a))
            finally:
                _lib.set_option("resize_vector", 1)
            case["a_call"] = stats(measure(lambda: [fusion.resize_probs_device(s, (W, H), **kw) for s in small]))

            # b: fusion with resampling inside the call against fusion of the images resampled beforehand (`outs`, from leg a)
            agg = fusion.MeshAggregator(P, C)
            b_resize = measure(lambda: agg.fuse_views(r, cams, small, resize="bilinear", **kw))
            b_plain = measure(lambda: agg.fuse_views(r, cams, outs, **kw))
            kernel = statistics.median([fuse_kernel_ms(lambda: agg.fuse_views(r, cams, outs, **kw)) for _ in range(REPS)])
            added = statistics.median(b_resize) - statistics.median(b_plain)
            case["b"] = {"fuse_views_resize": stats(b_resize), "fuse_views_preresampled": stats(b_plain), "added_us_per_view": 1e3 * added,
                         "fusion_kernel_us_per_view": 1e3 * kernel, "added_over_fusion_kernel": added / kernel if kernel else None}

            # c: host images
            small_host = [np.asarray(s) for s in small]
            big_host = [np.asarray(o) for o in outs]
            case["c"] = {"source_size_host_with_resize": stats(measure(lambda: agg.fuse_views(r, cams, small_host, resize="bilinear", **kw), warm=1)),
                         "full_size_host": stats(measure(lambda: agg.fuse_views(r, cams, big_host, **kw), warm=1)),
                         "host_bytes_per_image": [w * h * C * ITEM[dtype], W * H * C * ITEM[dtype]]}
            del big_host

            # d: torch on the device
            if torch is not None and dtype != "bfloat16":      # (bfloat16 device arrays are uint16 bit patterns here: not a torch dtype by this protocol)
                try:
                    tsmall = [torch.as_tensor(s, device="cuda").permute(2, 1, 0).contiguous()[None] for s in small]      # (1, C, h, w)

                    def torch_images():
                        return [torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0].permute(2, 1, 0).contiguous()
                                for t in tsmall]

                    def leg_d():
                        agg.fuse_views(r, cams, torch_images(), **kw)
                        torch.cuda.synchronize()
                    ref = np.asarray(outs[0]).astype(np.float32)
                    got = torch_images()[0].float().cpu().numpy()
                    case["d"] = dict(stats(measure(leg_d, warm=1)), max_abs_difference_from_a=float(np.abs(got - ref).max()))
                    del tsmall
                except Exception as e:      # (a torch build that cannot take this library's arrays: say so, measure the rest)
                    case["d"] = "not measured: %s: %s" % (type(e).__name__, e)
            else:
                case["d"] = "not measured"

            # e: scoring
            cm1, cm2 = fusion.ConfusionMatrix(C), fusion.ConfusionMatrix(C)
            e_one = measure(lambda: [cm1.add_probs(s, gt, resize="bilinear", **kw) for s in small])
            e_two = measure(lambda: [cm2.add_probs(fusion.resize_probs_device(s, (W, H), out_dtype="float32", **kw), gt) for s in small])
            equal = bool(np.array_equal(cm1.get(), cm2.get()))
            if not equal:
                raise SystemExit("leg e: the matrices differ (%s, %s)" % (g["name"], dtype))
            case["e"] = {"add_probs_resize": stats(e_one), "resize_then_add_probs": stats(e_two), "matrices_equal": equal}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del small, outs, small_host
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
