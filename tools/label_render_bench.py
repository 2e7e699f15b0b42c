"""The fused mesh rendered back into the views (fusion.LabelRenderer.render_views) at cfg2 -- 1 M triangles, 1080p --, 16 views per
call, with 19 and 150 classes, in both layouts, labels only and labels plus colours, left on the device and copied to the host.

Per view: the whole call between two marks on the library's stream (smesh_stream_mark; profiling off), and, in runs of their own with
the library's HIP-event profile slots on, the rasteriser (SMESH_PROF_RASTER) and the image kernel (SMESH_PROF_LABEL_IMAGES)
separately.  Bytes of the image kernel: 4 W H read plus the output bytes written, against 8 TB/s.
Beside it, in the same run, the route without this interface: render() + ModelRenderer.render_device() + copy to the host + numpy
argmax + palette + transpose, on a host clock, with the images checked equal.
usage: python tools/label_render_bench.py [output file, default profiles/label_render_bench.json]"""
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

VIEWS, REPS, PEAK = 16, 7, 8.0e12


def slot(which):
    ms, n, launches, views = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().smesh_profile_read_ex(0, which, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(launches), ctypes.byref(views)))
    return ms.value, int(launches.value)


def one_call(lr, renderer, cams, colors, on_device, profiled):
    """Milliseconds per view of one render_views call: (whole call, rasteriser, image kernel), and the image kernel's launches; the
    last three only when profiled."""
    lib = _lib.lib()
    _lib.check(lib.smesh_profile_enable(0, ((1 << _lib.PROF_RASTER) | (1 << _lib.PROF_LABEL_IMAGES)) if profiled else 0))
    _lib.check(lib.smesh_profile_reset(0))
    _lib.check(lib.smesh_stream_mark(0, 0))
    out = (lr.render_views_device if on_device else lr.render_views)(renderer, cams, colors=colors)
    _lib.check(lib.smesh_stream_mark(0, 1))
    _lib.synchronize(0)
    ms = ctypes.c_double()
    _lib.check(lib.smesh_stream_mark_elapsed(0, 0, 1, ctypes.byref(ms)))
    raster, (kernel, launches) = slot(_lib.PROF_RASTER)[0], slot(_lib.PROF_LABEL_IMAGES)
    _lib.check(lib.smesh_profile_enable(0, 0))
    del out
    n = len(cams)
    return ms.value / n, raster / n, kernel / n, launches


def measure(lr, renderer, cams, colors, on_device):
    samples = {False: [], True: []}
    for rep in range(REPS + 1):                    # (the first round warms up and is dropped)
        for prof in (False, True):
            t = one_call(lr, renderer, cams, colors, on_device, prof)
            if rep:
                samples[prof].append(t)
    whole = [s[0] for s in samples[False]]
    kern = [s[2] for s in samples[True]]
    return {"call_us_per_view": 1e3 * statistics.median(whole), "call_us_per_view_min_max": [1e3 * min(whole), 1e3 * max(whole)],
            "raster_us_per_view": 1e3 * statistics.median(s[1] for s in samples[True]),
            "kernel_us_per_view": 1e3 * statistics.median(kern), "kernel_us_per_view_min_max": [1e3 * min(kern), 1e3 * max(kern)],
            "kernel_launches_per_call": samples[True][0][3]}


def host_route(agg, renderer, cams, palette, C):
    """Seconds per view of the route without LabelRenderer: the (W,H,C) float image to the host, argmax, palette and transpose in numpy."""
    mr = agg.renderer()
    labels, colors = [], []
    t0 = time.perf_counter()
    for cam in cams:
        idx, _ = renderer.render(cam)
        image = mr.render_device(idx).numpy()
        pred = image.argmax(axis=-1).astype(np.uint8)
        total = np.zeros(image.shape[:2], np.float32)             # the rule of labels_device(): float32, ascending class order
        for c in range(C):
            total += image[..., c]
        care = total >= np.float32(0.9)
        pred[~care] = 255
        rgb = np.where(care[..., None], palette[np.where(care, pred, 0)], np.uint8(0))
        labels.append(np.ascontiguousarray(pred.T))
        colors.append(np.ascontiguousarray(rgb.transpose(1, 0, 2)))
    return (time.perf_counter() - t0) / len(cams), labels, colors


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "label_render_bench.json")
    cfg = synth.CONFIGS["cfg2"]
    mesh = synth.grid_mesh(cfg["a"], cfg["b"])
    W, H = cfg["width"], cfg["height"]
    cams = [synth.ring_camera(k, cfg["views"], W, H) for k in range(VIEWS)]
    renderer = render.triangles(mesh)
    P, N = len(mesh.faces), W * H
    result = {"tool": "tools/label_render_bench.py", "mesh_triangles": P, "width": W, "height": H, "views_per_call": VIEWS, "reps": REPS,
              "roofline_bytes_per_s": PEAK, "cases": []}
    for C in (19, 150):
        rng = np.random.default_rng(C)
        agg = fusion.MeshAggregator(P, C)
        step = 250000
        for lo in range(0, P, step):                                     # (raw state in pieces: no P*C host array at once)
            raw = rng.random((min(step, P - lo), C), dtype=np.float32) ** 8
            raw[rng.random(len(raw)) < 0.1] = 0.0
            agg.set_raw_rows(lo, raw)
        labels = agg.labels_device(0.9)
        palette = rng.integers(0, 256, size=(C, 3)).astype(np.uint8)
        case = {"classes": C, "runs": []}
        for layout in ("HW", "WH"):
            t0 = time.perf_counter()
            lr = fusion.LabelRenderer(labels, C, palette=palette, layout=layout)
            _lib.synchronize(0)
            create_ms = 1e3 * (time.perf_counter() - t0)
            for colors in (False, True):
                out_bytes = N * (1 + (3 if colors else 0))
                for on_device in (True, False):
                    m = measure(lr, renderer, cams, colors, on_device)
                    m.update({"layout": layout, "outputs": "labels+colours" if colors else "labels", "output_memory": "device" if on_device else "host",
                              "create_ms_host_clock": create_ms, "kernel_bytes_per_view": 4 * N + out_bytes})
                    m["kernel_bytes_per_s"] = m["kernel_bytes_per_view"] / (m["kernel_us_per_view"] * 1e-6)
                    m["kernel_share_of_roofline"] = m["kernel_bytes_per_s"] / PEAK
                    case["runs"].append(m)
            if layout == "HW":
                nviews = 1 if C > 40 else 2
                got_l, got_c = lr.render_views(renderer, cams[:nviews], colors=True)
                sec, want_l, want_c = host_route(agg, renderer, cams[:nviews], palette, C)
                case["host_route_ms_per_view"] = 1e3 * sec
                case["host_route_views"] = nviews
                case["host_route_image_bytes_per_view"] = N * C * 4
                case["host_route_images_equal_device"] = bool(all(np.array_equal(a, b) for a, b in zip(got_l, want_l))
                                                              and all(np.array_equal(a, b) for a, b in zip(got_c, want_c)))
                ref = next(r for r in case["runs"] if r["layout"] == "HW" and r["outputs"] == "labels+colours" and r["output_memory"] == "host")
                case["host_route_over_render_views_host"] = case["host_route_ms_per_view"] * 1e3 / ref["call_us_per_view"]
            del lr
        result["cases"].append(case)
        print(json.dumps(case))
        del agg, labels
        device.trim()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
