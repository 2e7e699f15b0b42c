"""Segments of a labelled mesh (fusion.FaceGraph.segments, fusion.FaceSegments) on synth's 1 M-triangle mesh, labels already on the
device: `segments` for constant labels (one giant segment), for 32 x 32-quad blocks of 19 labels, for those blocks with 3 % of the
faces re-labelled at random (the real case) and the same with normal weights; `despeckle_labels_device`; `despeckle_sums_device` +
`fill_labels_device(T = 32)` from an aggregator at 19 and 40 classes; and the route without this interface, once: labels and
adjacency on the host, then scipy.sparse.csgraph.connected_components where scipy imports, else the flood fill of
tests/face_segments_ref.py, with its ids compared to the device's.  Beside every time stand the bytes the call's kernels have to
move at the least (every array they read or write counted once per kernel) and what share of 8 TB/s that is.  Timed by a host
clock around smesh_synchronize; medians of REPS repeats with min - max, after one warm-up call.
usage: python tools/face_segments_bench.py [output file, default profiles/face_segments_bench.json]
       python tools/face_segments_bench.py --kernels    one untimed pass of the device calls, for
                                                        `rocprofv3 --kernel-trace --stats -- python tools/face_segments_bench.py --kernels`"""
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
T_FILL = 32
MIN_FACES = 50
MIN_WEIGHT = 0.5
GRID = (1000, 500)                                                   # the 1 M-triangle mesh of synth (cfg2)


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


def with_bytes(run, kernels):
    """`run` with the least bytes of each kernel of the call and the call's share of the peak."""
    total = float(sum(kernels.values()))
    run = dict(run, least_bytes_per_kernel=kernels, least_bytes=total)
    run["tb_per_s"] = total / (run["median_ms"] * 1e-3) / 1e12
    run["share_of_8_tb_per_s"] = run["tb_per_s"] / PEAK_TBS
    return run


def segments_bytes(F, nnz, S, weighted):
    """Every array a kernel reads or writes, once: the lists (offsets, neighbours, weights), labels, parent, root, flags, numbers."""
    lists = 4.0 * (F + 1) + 4.0 * nnz * (2 if weighted else 1)
    return {"labels copy": 8.0 * F,
            "k_seg_init": lists + 4.0 * F + 4.0 * F,                 # labels read, parent written (neighbours' labels: gathers of the same array)
            "k_seg_hook": lists + 4.0 * F + 4.0 * F,                 # labels and parent read; every union also writes a parent
            "k_seg_flatten": 4.0 * F * 4,                            # parent and labels read, root and flag written
            "scan (3 kernels)": 4.0 * F * 4,                         # flags read, numbers written, read and written again
            "k_seg_number": 4.0 * F * 4 + 12.0 * S}                  # root, numbers, labels read, ids written; the per-segment arrays


def block_labels(side=32, K=19):
    a, b = GRID
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    return np.repeat((((i // side) * 7 + (j // side) * 3) % K).astype(np.int32).reshape(-1), 2)


def canonical(component, labelled):
    """Component numbers of any numbering as the header's: -1 where unlabelled, else numbered in the order of the lowest face."""
    ids = np.full(len(component), -1, np.int64)
    faces = np.flatnonzero(labelled)
    uniq, first, inverse = np.unique(component[faces], return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    ids[faces] = rank[inverse]
    return ids.astype(np.int32)


def host_route(graph, d_labels):
    """Labels and adjacency to the host, components there; (seconds per step, ids)."""
    t0 = time.perf_counter()
    labels = d_labels.numpy()
    offsets, nbr = graph.adjacency()
    t1 = time.perf_counter()
    try:
        import scipy.sparse
        import scipy.sparse.csgraph
        how = "scipy.sparse.csgraph.connected_components"
        f = np.repeat(np.arange(len(labels), dtype=np.int64), np.diff(offsets.astype(np.int64)))
        g = nbr.astype(np.int64)
        ok = (labels[f] >= 0) & (labels[f] == labels[g])
        n = len(labels)
        m = scipy.sparse.csr_matrix((np.ones(int(ok.sum()), np.int8), (f[ok], g[ok])), shape=(n, n))
        component = scipy.sparse.csgraph.connected_components(m, directed=False)[1]
        ids = canonical(component, labels >= 0)
    except ImportError:
        import face_segments_ref
        how = "tests/face_segments_ref.py (scipy does not import)"
        ids = face_segments_ref.segments(offsets, nbr, labels)[0]
    t2 = time.perf_counter()
    return dict(how=how, to_host_s=t1 - t0, components_s=t2 - t1, repeats=1), ids


def main():
    kernels_only = "--kernels" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "face_segments_bench.json")
    mesh = synth.grid_mesh(*GRID)
    F, V = len(mesh.faces), len(mesh.vertices)
    rng = np.random.default_rng(0)
    graph = fusion.FaceGraph.from_mesh(mesh)
    nnz = graph.num_entries
    weights = graph.normal_weights(mesh.vertices)
    constant = np.full(F, 5, np.int32)
    blocks = block_labels()
    noisy = blocks.copy()
    hit = rng.random(F) < 0.03
    noisy[hit] = rng.integers(0, 19, int(hit.sum()))
    legs = {"constant": constant, "blocks": blocks, "blocks_3pct_noise": noisy}
    d_labels = {k: device.to_device(v) for k, v in legs.items()}

    def rows_of(C):
        rows = (rng.random((F, C), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
        rows[np.arange(F), noisy] += np.float32(1.0)
        rows /= rows.sum(axis=1, keepdims=True)
        rows[rng.random(F) < 0.1] = 0.0                               # faces no view observed
        return rows

    def aggregator_of(C):
        rows_h = rows_of(C)
        agg = fusion.MeshAggregator(F, C)
        for lo in range(0, F, 250000):
            agg.set_raw_rows(lo, rows_h[lo:lo + 250000])
        return agg

    if kernels_only:
        for name in legs:
            graph.segments(d_labels[name])
        seg = graph.segments(d_labels["blocks_3pct_noise"], weights=weights, min_weight=MIN_WEIGHT)
        seg.despeckle_labels_device(MIN_FACES)
        for C in (19, 40):
            agg = aggregator_of(C)
            seg = graph.segments(agg)
            graph.fill_labels_device(seg.despeckle_sums_device(agg, MIN_FACES), iterations=T_FILL)
        _lib.synchronize(0)
        return

    result = dict(tool="tools/face_segments_bench.py", timing="host clock around smesh_synchronize; median of %d after a warm-up" % REPS,
                  faces=F, vertices=V, entries=nnz, min_faces=MIN_FACES, min_weight=MIN_WEIGHT,
                  not_measured=["cfg5's 20 M faces", "real scans", "meshes whose face order is not spatially coherent"])

    def save():
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    for name in legs:
        seg = graph.segments(d_labels[name])
        r = with_bytes(timed(lambda: graph.segments(d_labels[name])), segments_bytes(F, nnz, seg.count, False))
        r.update(segments=seg.count, largest=int(seg.sizes().max()))
        result["segments_" + name] = r
        print(name, json.dumps(r, sort_keys=True), flush=True)
    seg_w = graph.segments(d_labels["blocks_3pct_noise"], weights=weights, min_weight=MIN_WEIGHT)
    r = with_bytes(timed(lambda: graph.segments(d_labels["blocks_3pct_noise"], weights=weights, min_weight=MIN_WEIGHT)),
                   segments_bytes(F, nnz, seg_w.count, True))
    r.update(segments=seg_w.count, largest=int(seg_w.sizes().max()))
    result["segments_blocks_3pct_noise_normal_weights"] = r
    print("weights", json.dumps(r, sort_keys=True), flush=True)
    seg = graph.segments(d_labels["blocks_3pct_noise"])
    out, faces_gone, segs_gone = seg.despeckle_labels_device(MIN_FACES, return_removed=True)
    r = with_bytes(timed(lambda: seg.despeckle_labels_device(MIN_FACES)), {"k_seg_despeckle_labels": 4.0 * F * 3 + 4.0 * seg.count})
    r.update(removed_faces=faces_gone, removed_segments=segs_gone)
    result["despeckle_labels_device"] = r
    print("despeckle", json.dumps(r, sort_keys=True), flush=True)
    save()
    for C in (19, 40):
        agg = aggregator_of(C)
        seg_a = graph.segments(agg)
        r = {"segments_from_aggregator": dict(timed(lambda: graph.segments(agg)), segments=seg_a.count),
             "despeckle_sums_device": with_bytes(timed(lambda: seg_a.despeckle_sums_device(agg, MIN_FACES)),
                                                 {"k_seg_despeckle_rows": 8.0 * F * C + 4.0 * F + 4.0 * seg_a.count}),
             "despeckle_sums_then_fill_labels_T32": timed(
                 lambda: graph.fill_labels_device(seg_a.despeckle_sums_device(agg, MIN_FACES), iterations=T_FILL)),
             "fill_labels_T32_alone": timed(lambda: graph.fill_labels_device(agg, iterations=T_FILL))}
        result["C%d" % C] = r
        print("C=%d" % C, json.dumps(r, sort_keys=True), flush=True)
        del agg, seg_a
        device.trim()
        save()
    # the route without this interface, once
    route, ids = host_route(graph, d_labels["blocks_3pct_noise"])
    route["ids_equal_device"] = bool(np.array_equal(ids, seg.ids()))
    result["host_route_blocks_3pct_noise"] = route
    print("host", route, flush=True)
    save()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
