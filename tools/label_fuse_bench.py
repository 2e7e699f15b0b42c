"""Label-image fusion against its one-hot equivalent at BASELINE cfg2's geometry, eight views per call:

  (a) fuse_views        on one-hot float32 (W,H,C) class vectors   -- what the reference's colorize_mesh.py:39-67 builds
  (b) fuse_views_labels on the uint8 masks of the same labels

each with device-resident and with host-resident inputs.  Per leg: `--regions` timed regions of `--calls` calls (eight views each)
after `--warmup` calls; views/s as the median over the regions with their min-max range, and the fusion slot's HIP-event time per
launch (smesh_profile_*) from a separate profiled pass (the event pairs cost stream time, so they are not in the timed regions).
`--legs a` runs the one-hot legs only: that is all a build without the label entry points can run, and the yardstick of (b).

    python tools/label_fuse_bench.py [--legs ab] [--regions 7] [--calls 6] [--warmup 3] [--host-calls 2]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_meshes_amd import _lib, fusion, render, synth  # noqa: E402
from semantic_meshes_amd.device import to_device  # noqa: E402

GROUP = 8


def fuse_slot():
    ms, n = ctypes.c_double(), ctypes.c_uint64()
    _lib.check(_lib.lib().smesh_profile_read(0, _lib.PROF_FUSE_SCATTER, ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value


def run_leg(name, call, regions, calls, warmup):
    for _ in range(warmup):
        call()
    _lib.synchronize(0)
    rates = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        _lib.synchronize(0)
        rates.append(calls * GROUP / (time.perf_counter() - t0))
    _lib.check(_lib.lib().smesh_profile_reset(0))
    _lib.check(_lib.lib().smesh_profile_enable(0, 1 << _lib.PROF_FUSE_SCATTER))
    for _ in range(max(calls, 2)):
        call()
    _lib.synchronize(0)
    ms, n = fuse_slot()
    _lib.check(_lib.lib().smesh_profile_enable(0, 0))
    kernel = _lib.last_fuse_kernel()
    print("%-28s %9.1f views/s median of %d regions (min %.1f, max %.1f); fusion slot %.1f us per region of %d views, %d regions [%s]"
          % (name, statistics.median(rates), regions, min(rates), max(rates), 1e3 * ms / max(n, 1), GROUP, n, kernel), flush=True)
    return statistics.median(rates), min(rates), max(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--classes", default="", help="comma-separated class counts for further device-resident label legs (c) on the same views")
    args = ap.parse_args()
    mesh, cams, C = synth.scene("cfg2")
    P = len(mesh.faces)
    W, H = cams[0].resolution
    views = [5, 31, 57, 83, 109, 135, 161, 187]
    group = [cams[k] for k in views]
    rng = np.random.default_rng(2024)
    masks = []
    for _ in views:
        m = rng.integers(0, C, size=(W, H), dtype=np.uint8)
        m[rng.random((W, H)) < 0.03] = 255
        masks.append(m)
    r = render.triangles(mesh)
    print("cfg2: %d triangles, %d x %d, C = %d, %d views per call; one-hot view %.1f MB, mask %.2f MB"
          % (P, W, H, C, GROUP, W * H * C * 4 / 1e6, W * H / 1e6), flush=True)
    if "a" in args.legs:
        eye = np.eye(C + 1, C, dtype=np.float32)                  # row C: the all-zero don't-care vector
        hot = [eye[np.minimum(m, C)] for m in masks]
        d_hot = [to_device(h) for h in hot]
        agg = fusion.MeshAggregator(P, C)
        run_leg("(a) one-hot, device", lambda: agg.fuse_views(r, group, d_hot), args.regions, args.calls, args.warmup)
        run_leg("(a) one-hot, host", lambda: agg.fuse_views(r, group, hot), max(3, args.regions // 2), args.host_calls, 1)
        del d_hot, hot
    if "b" in args.legs:
        d_masks = [to_device(m) for m in masks]
        agg = fusion.MeshAggregator(P, C)
        run_leg("(b) uint8 labels, device", lambda: agg.fuse_views_labels(r, group, d_masks), args.regions, args.calls, args.warmup)
        run_leg("(b) uint8 labels, host", lambda: agg.fuse_views_labels(r, group, masks), max(3, args.regions // 2), args.host_calls, 1)
        del agg
        for Cx in [int(c) for c in args.classes.split(",") if c]:
            # the same kernel at other class counts: rows in LDS up to 255 classes, read-modify-write in global memory beyond
            wide = [to_device((rng.integers(0, Cx, size=(W, H)) % 256).astype(np.uint8)) for _ in views]
            aggx = fusion.MeshAggregator(P, Cx)
            run_leg("(c) uint8 labels, C = %d" % Cx, lambda: aggx.fuse_views_labels(r, group, wide), args.regions, args.calls, args.warmup)
            del aggx, wide


if __name__ == "__main__":
    main()
