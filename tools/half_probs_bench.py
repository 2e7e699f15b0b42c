"""float16 / bfloat16 class-vector fusion against float32 at BASELINE cfg2's geometry (its mesh at 1920 x 1080), Sum, 16 device-resident
views per fuse_views call, at 19 and 40 classes.  In ONE run:

  (a) float32 images through smesh_fuse_views                       -- k_fuse_tri
  (b) the same images narrowed to float16 and to bfloat16           -- k_fuse_tri_h16 reads them in place
  (c) the 16-bit images through the widening route (SMESH_FUSE_H16=0: a group's images widened by k_widen_probs16 into scratch slots, then
      smesh_fuse_views' own path for the group: k_fuse_tri, eight views per launch)

Before timing, (b) and (c) must give raw accumulators bit-equal to the float32 path on the widened images.  Per leg: the whole-call
time per view (wall clock around the call and a synchronize, group pipeline as configured) and, with the group pipeline off, the
fusion kernels' time per view from the library's HIP-event slot -- medians of `--calls` calls with their min-max range --, the bytes
the kernel needs per view (class vectors of the visible pixels, one record per triangle, each accumulator row read and written once per
launch) and the fraction of 8 TB/s that comes to.  For (c) the slot times the float32 kernel only: the widening shows in the whole call.

    python tools/half_probs_bench.py [--classes 19,40] [--views 16] [--calls 7] [--warmup 2] [--out profiles/half_probs_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_meshes_amd import _lib, fusion, render, synth  # noqa: E402
from semantic_meshes_amd.device import to_device  # noqa: E402

PEAK = 8e12      # bytes / s


def widen(bits16, dtype):
    if dtype == "float16":
        return bits16.view(np.float16).astype(np.float32)
    return (bits16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def slot_read():
    ms, regions, launches, views = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().smesh_profile_read_ex(0, _lib.PROF_FUSE_SCATTER, ctypes.byref(ms), ctypes.byref(regions), ctypes.byref(launches),
                                                ctypes.byref(views)))
    return ms.value, int(launches.value), int(views.value)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def run_leg(name, call, nviews, calls, warmup, bytes_per_view):
    for _ in range(warmup):
        call()
    _lib.synchronize(0)
    whole = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        _lib.synchronize(0)
        whole.append(1e6 * (time.perf_counter() - t0) / nviews)
    pipeline = _lib.get_option("group_pipeline")
    _lib.set_option("group_pipeline", 0)           # the kernel's own duration: no rasteriser beside it
    kernel, per_launch = [], 0
    try:
        call()
        _lib.synchronize(0)
        _lib.check(_lib.lib().smesh_profile_enable(0, 1 << _lib.PROF_FUSE_SCATTER))
        for _ in range(calls):
            _lib.check(_lib.lib().smesh_profile_reset(0))
            call()
            _lib.synchronize(0)
            ms, launches, views = slot_read()
            kernel.append(1e3 * ms / max(views, 1))
            per_launch = views / max(launches, 1)
    finally:
        _lib.check(_lib.lib().smesh_profile_enable(0, 0))
        _lib.set_option("group_pipeline", pipeline)
    name_k = _lib.last_fuse_kernel()
    k = spread(kernel)
    res = {"leg": name, "kernel": name_k, "views_per_launch": per_launch, "whole_call_us_per_view": spread(whole),
           "kernel_us_per_view": k, "kernel_bytes_per_view": bytes_per_view,
           "fraction_of_8TBs": bytes_per_view / (k["median"] * 1e-6) / PEAK}
    print("%-34s whole call %7.1f us/view (%.1f - %.1f)   kernel %6.1f us/view (%.1f - %.1f)   %6.1f MB/view   %4.1f %% of 8 TB/s   [%s, %g views/launch]"
          % (name, res["whole_call_us_per_view"]["median"], min(whole), max(whole), k["median"], k["min"], k["max"], bytes_per_view / 1e6,
             100 * res["fraction_of_8TBs"], name_k, per_launch), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="19,40")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "half_probs_bench.json"))
    args = ap.parse_args()
    os.environ.pop("SMESH_FUSE_H16", None)
    mesh, cams, _ = synth.scene("cfg2")
    P = len(mesh.faces)
    W, H = cams[0].resolution
    step = max(1, len(cams) // args.views)
    group = [cams[(5 + k * step) % len(cams)] for k in range(args.views)]
    r = render.triangles(mesh)
    visible = float(np.mean([(np.asarray(r.render(cam)[0]) != 0xFFFFFFFF).sum() for cam in group[:4]]))
    print("cfg2 mesh: %d triangles, %d x %d, %d views per call, %.0f visible pixels per view" % (P, W, H, args.views, visible), flush=True)
    out = {"mesh_triangles": P, "width": W, "height": H, "views_per_call": args.views, "calls": args.calls, "aggregator": "sum",
           "visible_pixels_per_view": visible, "bytes_model": "visible * C * itemsize + 16 * F + 2 * F * C * 4 / views_per_launch", "classes": {}}
    for C in [int(c) for c in args.classes.split(",") if c]:
        f32 = [synth.device_probs(W, H, C, synth.probs_seed(7, k), 0.03, 0) for k in range(args.views)]
        f16 = [fusion.narrow_probs(p, "float16") for p in f32]
        bf16 = [fusion.narrow_probs(p, "bfloat16") for p in f32]
        _lib.synchronize(0)
        # ---- the check: raw accumulators of (b) and (c) against the float32 path on the widened images, bit for bit
        for dtype, imgs in (("float16", f16), ("bfloat16", bf16)):
            ref = fusion.MeshAggregator(P, C)
            for lo in range(0, args.views, 4):      # (four widened float32 images on the device at a time)
                wide = [to_device(widen(np.asarray(i).view(np.uint16), dtype)) for i in imgs[lo:lo + 4]]
                ref.fuse_views(r, group[lo:lo + 4], wide)
            want = ref.get_raw().view(np.uint32)
            assert want.any()
            for hook, kernel in ((None, "k_fuse_tri_h16"), ("0", "k_fuse_tri")):
                if hook is None:
                    os.environ.pop("SMESH_FUSE_H16", None)
                else:
                    os.environ["SMESH_FUSE_H16"] = hook
                agg = fusion.MeshAggregator(P, C)
                for lo in range(0, args.views, 4):
                    agg.fuse_views(r, group[lo:lo + 4], imgs[lo:lo + 4])
                assert _lib.last_fuse_kernel() == kernel, _lib.last_fuse_kernel()
                if not np.array_equal(agg.get_raw().view(np.uint32), want):
                    raise SystemExit("C = %d %s SMESH_FUSE_H16=%s: raw accumulator differs from the float32 path on the widened images" % (C, dtype, hook))
            os.environ.pop("SMESH_FUSE_H16", None)
            del ref, agg, wide
        print("C = %d: (b) and (c) bit-equal to the float32 path on the widened images, both dtypes" % C, flush=True)

        def need(itemsize, per_launch):
            return visible * C * itemsize + 16 * P + 2 * P * C * 4 / per_launch
        legs = []
        agg = fusion.MeshAggregator(P, C)
        legs.append(run_leg("C=%d (a) float32" % C, lambda: agg.fuse_views(r, group, f32), args.views, args.calls, args.warmup, need(4, 8)))
        legs.append(run_leg("C=%d (b) float16, k_fuse_tri_h16" % C, lambda: agg.fuse_views(r, group, f16), args.views, args.calls, args.warmup, need(2, 8)))
        legs.append(run_leg("C=%d (b) bfloat16, k_fuse_tri_h16" % C, lambda: agg.fuse_views(r, group, bf16), args.views, args.calls, args.warmup, need(2, 8)))
        os.environ["SMESH_FUSE_H16"] = "0"
        try:
            legs.append(run_leg("C=%d (c) float16, widened" % C, lambda: agg.fuse_views(r, group, f16), args.views, args.calls, args.warmup, need(4, 8)))
            legs.append(run_leg("C=%d (c) bfloat16, widened" % C, lambda: agg.fuse_views(r, group, bf16), args.views, args.calls, args.warmup, need(4, 8)))
        finally:
            os.environ.pop("SMESH_FUSE_H16", None)
        a, b = legs[0]["kernel_us_per_view"], [leg["kernel_us_per_view"] for leg in legs[1:3]]
        out["classes"][str(C)] = {"legs": legs, "kernel_speedup_b_over_a": [a["median"] / x["median"] for x in b],
                                  "whole_call_speedup_b_over_a": [legs[0]["whole_call_us_per_view"]["median"] / leg["whole_call_us_per_view"]["median"]
                                                                  for leg in legs[1:3]]}
        del agg, f32, f16, bf16
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
