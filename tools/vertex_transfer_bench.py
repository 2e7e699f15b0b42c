"""Per-vertex results (fusion.VertexTransfer): the map build, labels only and full annotations from an aggregator, timed with HIP
events on the library's stream (smesh_stream_mark), beside get_device() of the same aggregator -- both are single passes over the
same [F,C] rows, so the gather's time as a multiple of get_device()'s is the yardstick.
usage: python tools/vertex_transfer_bench.py [output file, default profiles/vertex_transfer.txt]"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, device, fusion, synth          # noqa: E402

REPS = 5


def timed(call):
    """(best milliseconds between two marks on the library's stream, host milliseconds of the same call) over REPS calls."""
    lib, best, host = _lib.lib(), float("inf"), float("inf")
    for _ in range(REPS + 1):          # (the first call allocates)
        _lib.check(lib.smesh_stream_mark(0, 0))
        t0 = time.perf_counter()
        out = call()
        _lib.check(lib.smesh_stream_mark(0, 1))
        _lib.synchronize(0)
        host = min(host, 1e3 * (time.perf_counter() - t0))
        del out
        ms = ctypes.c_double()
        _lib.check(lib.smesh_stream_mark_elapsed(0, 0, 1, ctypes.byref(ms)))
        best = min(best, ms.value)
    return best, host


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vertex_transfer.txt")
    lines = ["tools/vertex_transfer_bench.py: best of %d, milliseconds between two HIP events on the library's stream (host time in brackets)" % REPS,
             "gather bytes = F*C*4 read once + V*C*4 written (labels only: V*4 written)", ""]
    for name, a, b, C in (("cfg2 mesh", 1000, 500, 19), ("150 classes", 1000, 500, 150), ("150 classes, 4 M faces", 2000, 1000, 150)):
        mesh = synth.grid_mesh(a, b)
        F, V = len(mesh.faces), len(mesh.vertices)
        rng = np.random.default_rng(C)
        agg = fusion.MeshAggregator(F, C)
        step = 250000
        for lo in range(0, F, step):                                     # (raw state in pieces: no F*C host array at once)
            raw = rng.random((min(step, F - lo), C), dtype=np.float32)
            raw[rng.random(len(raw)) < 0.3] = 0.0
            agg.set_raw_rows(lo, raw)
        build, build_host = timed(lambda: fusion.VertexTransfer.from_mesh(mesh))
        vt = fusion.VertexTransfer.from_mesh(mesh)
        get, get_host = timed(agg.get_device)
        lab, lab_host = timed(lambda: vt.labels_device(agg))
        ann, ann_host = timed(lambda: vt.annotations_device(agg))
        rows = agg.get_device()
        g_lab, _ = timed(lambda: vt.labels_device(rows))                 # the gather alone: rows already final
        g_ann, _ = timed(lambda: vt.annotations_device(rows))
        t_get = t_lab = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            host_rows = agg.get()
            t_get = min(t_get, 1e3 * (time.perf_counter() - t0))
            del host_rows
            t0 = time.perf_counter()
            host_labels = vt.labels(agg)                                  # int32 [V] on the HOST, like get()'s result
            t_lab = min(t_lab, 1e3 * (time.perf_counter() - t0))
            del host_labels
        del rows
        rd, wr = F * C * 4.0, V * C * 4.0
        lines += [
            "%s: F = %d, V = %d, C = %d" % (name, F, V, C),
            "  map build                         %8.3f ms  (%.3f host; once per mesh)" % (build, build_host),
            "  get_device()                      %8.3f ms  (%.3f host)  %.2f TB/s over 2*F*C*4" % (get, get_host, 2 * rd / get / 1e9),
            "  gather, labels only               %8.3f ms  %.2f TB/s  = %.2f x get_device" % (g_lab, (rd + V * 4.0) / g_lab / 1e9, g_lab / get),
            "  gather, annotations               %8.3f ms  %.2f TB/s  = %.2f x get_device" % (g_ann, (rd + wr) / g_ann / 1e9, g_ann / get),
            "  aggregator -> labels (device)     %8.3f ms  (%.3f host)  finalise + gather" % (lab, lab_host),
            "  aggregator -> annotations (dev.)  %8.3f ms  (%.3f host)  finalise + gather" % (ann, ann_host),
            "  labels(agg) to the host           %8.3f ms host" % t_lab,
            "  get() to the host alone           %8.3f ms host: what the host path pays BEFORE its adjacency loop and gather start" % t_get,
            "  labels on the host from an aggregator are %s than get() followed by the host path (%.3f ms against %.3f ms + that path)" % (
                "cheaper" if t_lab < t_get else "NOT cheaper than get() alone, let alone", t_lab, t_get),
            ""]
        del agg, vt
        device.trim()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
