"""Confusion matrices on the device (fusion.ConfusionMatrix.add_views) at cfg2 -- 1 M triangles, 1080p -- with 19, 40 and 150
classes, against a random ground-truth image and a uniform one, with and without the counting kernel's in-wave aggregation.

Per view: the whole call between two marks on the library's stream (smesh_stream_mark; profiling off), and, in runs of their own with
the library's HIP-event profile slots on, the rasteriser (SMESH_PROF_RASTER) and the counting kernel (SMESH_PROF_CONFUSION)
separately.  Bytes of the counting kernel: N * (4 + bytes of a ground-truth element) + the label table once, against 8 TB/s.
Beside it, in the same run, the route without this interface: render() + ModelRenderer.render_device() + copy to the host + numpy
argmax + np.add.at, on a host clock.
usage: python tools/confusion_bench.py [output file, default profiles/confusion_bench.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, device, evaluation, fusion, render, synth          # noqa: E402

VIEWS, REPS, PEAK = 16, 7, 8.0e12


def slot(which):
    ms, n, launches, views = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().smesh_profile_read_ex(0, which, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(launches), ctypes.byref(views)))
    return ms.value, int(n.value)


def one_call(cm, renderer, cams, labels, gts, profiled):
    """Milliseconds per view of one add_views call: (whole call, rasteriser, counting kernel); the last two only when profiled."""
    lib = _lib.lib()
    cm.reset()
    _lib.check(lib.smesh_profile_enable(0, ((1 << _lib.PROF_RASTER) | (1 << _lib.PROF_CONFUSION)) if profiled else 0))
    _lib.check(lib.smesh_profile_reset(0))
    _lib.check(lib.smesh_stream_mark(0, 0))
    cm.add_views(renderer, cams, labels, gts)
    _lib.check(lib.smesh_stream_mark(0, 1))
    _lib.synchronize(0)
    ms = ctypes.c_double()
    _lib.check(lib.smesh_stream_mark_elapsed(0, 0, 1, ctypes.byref(ms)))
    raster, count = slot(_lib.PROF_RASTER)[0], slot(_lib.PROF_CONFUSION)[0]
    _lib.check(lib.smesh_profile_enable(0, 0))
    n = len(cams)
    return ms.value / n, raster / n, count / n


def measure(cm, renderer, cams, labels, gts):
    """Medians over REPS calls, aggregation on and off alternating call by call."""
    lib = _lib.lib()
    out = {}
    default = ctypes.c_int64(0)
    _lib.check(lib.smesh_get_option(b"confusion_wave_aggregate", ctypes.byref(default)))
    default = int(default.value)
    samples = {(agg, prof): [] for agg in (1, 0) for prof in (False, True)}
    for rep in range(REPS + 1):                    # (the first round warms up every shape and is dropped)
        for agg in (1, 0):
            _lib.check(lib.smesh_set_option(b"confusion_wave_aggregate", agg))
            for prof in (False, True):
                t = one_call(cm, renderer, cams, labels, gts, prof)
                if rep:
                    samples[(agg, prof)].append(t)
    _lib.check(lib.smesh_set_option(b"confusion_wave_aggregate", default))
    for agg in (1, 0):
        whole = [s[0] for s in samples[(agg, False)]]
        out["aggregate" if agg else "plain"] = {
            "call_us_per_view": 1e3 * statistics.median(whole), "call_us_per_view_min_max": [1e3 * min(whole), 1e3 * max(whole)],
            "raster_us_per_view": 1e3 * statistics.median(s[1] for s in samples[(agg, True)]),
            "count_us_per_view": 1e3 * statistics.median(s[2] for s in samples[(agg, True)]),
            "count_us_per_view_min_max": [1e3 * min(s[2] for s in samples[(agg, True)]), 1e3 * max(s[2] for s in samples[(agg, True)])]}
    return out


def host_route(agg, renderer, cams, gts_host, C):
    """Seconds per view of the route without ConfusionMatrix: the (W,H,C) float image to the host, argmax and np.add.at in numpy."""
    mr = agg.renderer()
    M = np.zeros((C, C + 1), np.uint64)
    t0 = time.perf_counter()
    for cam, gt in zip(cams, gts_host):
        idx, _ = renderer.render(cam)
        image = mr.render_device(idx).numpy()
        pred = image.argmax(axis=-1)
        pred[image.sum(axis=-1) < 0.9] = C
        ok = gt < C
        np.add.at(M, (gt[ok], pred[ok]), 1)
    return (time.perf_counter() - t0) / len(cams), M


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "confusion_bench.json")
    cfg = synth.CONFIGS["cfg2"]
    mesh = synth.grid_mesh(cfg["a"], cfg["b"])
    W, H = cfg["width"], cfg["height"]
    cams = [synth.ring_camera(k, cfg["views"], W, H) for k in range(VIEWS)]
    renderer = render.triangles(mesh)
    P, N = len(mesh.faces), W * H
    result = {"tool": "tools/confusion_bench.py", "mesh_triangles": P, "width": W, "height": H, "views_per_call": VIEWS, "reps": REPS,
              "roofline_bytes_per_s": PEAK, "lds_max_classes": evaluation.lds_max_classes(), "cases": []}
    for C in (19, 40, 150):
        rng = np.random.default_rng(C)
        agg = fusion.MeshAggregator(P, C)
        step = 250000
        for lo in range(0, P, step):                                     # (raw state in pieces: no P*C host array at once)
            raw = rng.random((min(step, P - lo), C), dtype=np.float32) ** 8
            raw[rng.random(len(raw)) < 0.1] = 0.0
            agg.set_raw_rows(lo, raw)
        t0 = time.perf_counter()
        labels = agg.labels_device(0.9)
        _lib.synchronize(0)
        labels_ms = 1e3 * (time.perf_counter() - t0)
        cm = fusion.ConfusionMatrix(C)
        bytes_per_view = N * (4 + 1) + P * 4
        case = {"classes": C, "labels_device_ms_host_clock": labels_ms, "count_bytes_per_view": bytes_per_view, "ground_truth": {}}
        for kind in ("random", "uniform"):
            if kind == "random":
                gts_host = [rng.integers(0, C, size=(W, H)).astype(np.uint8) for _ in cams]
                table = labels
            else:                                                         # every covered pixel in one bin, the background in a second
                gts_host = [np.full((W, H), 3, np.uint8) for _ in cams]
                table = device.to_device(np.full(P, 3, np.int32))
            gts = [device.to_device(g) for g in gts_host]
            m = measure(cm, renderer, cams, table, gts)
            for v in m.values():
                v["count_bytes_per_s"] = bytes_per_view / (v["count_us_per_view"] * 1e-6)
                v["count_share_of_roofline"] = v["count_bytes_per_s"] / PEAK
            case["ground_truth"][kind] = m
            if kind == "random":
                nviews = 1 if C > 40 else 2
                cm.reset()
                cm.add_views(renderer, cams[:nviews], labels, gts[:nviews])
                got = cm.get()
                sec, M = host_route(agg, renderer, cams[:nviews], gts_host[:nviews], C)
                case["host_route_ms_per_view"] = 1e3 * sec
                case["host_route_views"] = nviews
                case["host_route_image_bytes_per_view"] = N * C * 4
                case["host_route_matrix_equals_device"] = bool(np.array_equal(M, got))
            del gts
        result["cases"].append(case)
        print(json.dumps(case))
        del agg, cm, labels
        device.trim()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
