"""Smoothing and filling over the face graph (fusion.FaceGraph) on synth's 1 M-triangle mesh at 19 and 40 classes: the graph build,
smooth_labels_device at T = 10 with and without weights, fill_labels_device at T = 32, normal_weights, the time of one iteration
(the difference to the same call at T = 0, divided by T) beside the bytes an iteration has to move -- x_t and x0 read once, x_{t+1}
written once: 3 F C 4 -- as a share of 8 TB/s, and the route without this interface: the rows on the host, the adjacency and T
products in numpy (tests/face_graph_ref.py), once, with its labels compared to the device's.  Timed by a host clock around
smesh_synchronize; medians of REPS repeats with min - max, after one warm-up call.
usage: python tools/face_smooth_bench.py [output file, default profiles/face_smooth_bench.json]
       python tools/face_smooth_bench.py --kernels      one untimed pass of the device calls, for
                                                        `rocprofv3 --kernel-trace --stats -- python tools/face_smooth_bench.py --kernels`"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from semantic_meshes_amd import _lib, device, fusion, synth          # noqa: E402

REPS = 7
PEAK_TBS = 8.0
T_SMOOTH, T_FILL = 10, 32


def timed(call):
    """dict(median_ms, min_ms, max_ms, repeats) of `call`, each run bracketed by smesh_synchronize."""
    def once():
        _lib.synchronize(0)
        t0 = time.perf_counter()
        out = call()
        _lib.synchronize(0)
        ms = 1e3 * (time.perf_counter() - t0)
        del out
        return ms
    warm = once()
    ms = [once() for _ in range(REPS)]
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms), warm_up_ms=warm)


def per_iteration(run, base, T, F, C):
    us = 1e3 * (run["median_ms"] - base["median_ms"]) / T
    moved = 3.0 * F * C * 4
    return dict(iterations=T, us_per_iteration=us, bytes_per_iteration=moved, tb_per_s=moved / (us * 1e-6) / 1e12,
                share_of_8_tb_per_s=moved / (us * 1e-6) / 1e12 / PEAK_TBS)


def make_rows(rng, F, C):
    rows = rng.random((F, C), dtype=np.float32)
    rows /= rows.sum(axis=1, keepdims=True)
    rows[rng.random(F) < 0.3] = 0.0
    return rows


def main():
    kernels_only = "--kernels" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "face_smooth_bench.json")
    mesh = synth.grid_mesh(1000, 500)                                # the 1 M-triangle mesh of synth (cfg2)
    F, V = len(mesh.faces), len(mesh.vertices)
    rng = np.random.default_rng(0)
    graph = fusion.FaceGraph.from_mesh(mesh)
    weights = graph.normal_weights(mesh.vertices)
    if kernels_only:
        for C in (19, 40):
            rows = device.to_device(make_rows(rng, F, C))
            graph.smooth_labels_device(rows, T_SMOOTH)
            graph.smooth_labels_device(rows, T_SMOOTH, weights=weights)
            graph.fill_labels_device(rows, T_FILL)
        _lib.synchronize(0)
        return
    result = dict(tool="tools/face_smooth_bench.py", timing="host clock around smesh_synchronize; median of %d after a warm-up" % REPS,
                  faces=F, vertices=V, entries=graph.num_entries,
                  not_measured=["cfg5's 20 M faces", "real scans", "iteration counts other than 0, 10 and 32"])
    result["graph_build"] = timed(lambda: fusion.FaceGraph.from_mesh(mesh))
    result["normal_weights"] = timed(lambda: graph.normal_weights(mesh.vertices))

    def save():
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    host_rows = None
    for C in (19, 40):
        rows_h = make_rows(rng, F, C)
        rows = device.to_device(rows_h)
        r = {}
        r["labels_T0"] = timed(lambda: graph.smooth_labels_device(rows, 0))
        r["smooth_labels_T10"] = timed(lambda: graph.smooth_labels_device(rows, T_SMOOTH))
        r["smooth_labels_T10_weights"] = timed(lambda: graph.smooth_labels_device(rows, T_SMOOTH, weights=weights))
        r["fill_labels_T32"] = timed(lambda: graph.fill_labels_device(rows, T_FILL))
        r["smooth_iteration"] = per_iteration(r["smooth_labels_T10"], r["labels_T0"], T_SMOOTH, F, C)
        r["smooth_iteration_weights"] = per_iteration(r["smooth_labels_T10_weights"], r["labels_T0"], T_SMOOTH, F, C)
        r["fill_iteration"] = per_iteration(r["fill_labels_T32"], r["labels_T0"], T_FILL, F, C)
        agg = fusion.MeshAggregator(F, C)
        for lo in range(0, F, 250000):
            agg.set_raw_rows(lo, rows_h[lo:lo + 250000])
        r["smooth_labels_T10_from_aggregator"] = timed(lambda: graph.smooth_labels_device(agg, T_SMOOTH))
        r["get_device"] = timed(agg.get_device)
        del agg
        result["C%d" % C] = r
        print("C=%d" % C, json.dumps(r, sort_keys=True), flush=True)
        save()
        if C == 19:
            host_rows, host_dev_labels = rows_h, graph.smooth_labels_device(rows, T_SMOOTH).numpy()
        del rows
        device.trim()
    # the route without this interface, once: adjacency and T = 10 products in numpy
    import face_graph_ref
    t0 = time.perf_counter()
    offsets, nbr = face_graph_ref.adjacency(mesh.faces, V)
    t1 = time.perf_counter()
    x, tot = face_graph_ref.propagate(offsets, nbr, host_rows, T_SMOOTH, face_graph_ref.SMOOTH, alpha=0.5)
    labels = face_graph_ref.finish(x, tot, 0.9)[0]
    t2 = time.perf_counter()
    result["numpy_route_C19_T10"] = dict(adjacency_s=t1 - t0, propagate_s=t2 - t1, repeats=1,
                                         labels_equal_device=bool(np.array_equal(labels, host_dev_labels)),
                                         adjacency_equal_device=bool(np.array_equal(nbr, graph.adjacency()[1])))
    print("numpy", result["numpy_route_C19_T10"], flush=True)
    save()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
