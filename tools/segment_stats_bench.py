"""Fused rows pooled over segments (fusion.FaceSegments.members / pool_sums / pooled_face_labels / despeckle_labels_by) on synth's
1 M-triangle mesh, rows and labels already on the device.  Legs: the member-table build (a fresh FaceSegments per repeat: the table
is kept in the handle after its first use), `pool_sums_device`, `pooled_face_labels_device` and `despeckle_labels_by_device` (with
the table built).  Cases: constant labels (one giant segment, 3 907 chunks), 32 x 32-quad blocks of 19 labels, those blocks with
3 % of the faces re-labelled at random; 19 and 40 classes; from device rows and from an aggregator.  Beside every time stand the
bytes each kernel of the call has to move at the least (every array it reads or writes counted once) and what share of 8 TB/s that
is.  The route without this interface -- `get()`, `ids()`, `np.add.at` -- runs once; its sums add in another order, so the
comparison states the largest relative difference that was observed and is no parity claim.  Timed by a host clock around
smesh_synchronize; medians of REPS repeats with min - max, after one warm-up call.

THE SORT'S DIGIT WIDTH.  The member table is an LSD radix sort of the labelled faces by segment id; SMESH_SEGMENT_SORT_BITS picks the
digit: 1, a stable split per bit (flag, scan over all faces, scatter), or up to 4, a stable split per digit (per-tile counts by
ballot, a scan over 16 counts per tile, scatter).  The rule, written before any run: the simpler one-bit form stays unless the wider
one wins on the member-table leg by more than the repeats' min - max, in alternating runs.  `sort_digit_<labelling>` holds ROUNDS
alternating pairs and `wide_wins`: the wide form's slowest repeat below the one-bit form's fastest, in every pair.

usage: python tools/segment_stats_bench.py [output file, default profiles/segment_stats_bench.json]
       python tools/segment_stats_bench.py --kernels    one untimed pass of the device calls, for
                                                        `rocprofv3 --kernel-trace --stats -- python tools/segment_stats_bench.py --kernels`"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_meshes_amd import _lib, device, fusion, synth          # noqa: E402

REPS = 7
PEAK_TBS = 8.0
GRID = (1000, 500)                                                   # the 1 M-triangle mesh of synth (cfg2)
CHUNK = 256
SORT_ENV, WIDE_BITS, ROUNDS = "SMESH_SEGMENT_SORT_BITS", 4, 3          # the member table's sort: one bit against a 4-bit digit


def timed(call, setup=None):
    """dict(median_ms, min_ms, max_ms, repeats) of `call(setup())`, each run bracketed by smesh_synchronize; `setup` is not timed."""
    def once():
        arg = setup() if setup else None
        _lib.synchronize(0)
        t0 = time.perf_counter()
        out = call(arg) if setup else call()
        _lib.synchronize(0)
        ms = 1e3 * (time.perf_counter() - t0)
        del out, arg
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


def shape_of(sizes):
    """(chunks, partial rows) of segments of these sizes."""
    chunks = (sizes.astype(np.int64) + CHUNK - 1) // CHUNK
    return int(chunks.sum()), int(chunks[chunks > 1].sum())


def members_bytes(F, S, L):
    """The library's default: WIDE_BITS bits per pass; every pass reads the faces and their ids twice and writes the faces once."""
    bits = int(S - 1).bit_length() if S > 1 else 0
    passes = -(-bits // WIDE_BITS)
    tiles = -(-L // CHUNK)
    return {"k_ss_counts + 3 scans over S": 16.0 * S + 3 * 16.0 * S,
            "k_ss_labelled + scan + k_ss_compact": 8.0 * F + 16.0 * F + 8.0 * F + 4.0 * L,
            "%d x (k_ss_digit_count + scan + k_ss_digit_scatter)" % passes: passes * (8.0 * L + 12.0 * L + 5 * 4.0 * 16 * tiles),
            "copies out": 8.0 * (S + L)}


def pool_bytes(F, S, L, C, sizes, weighted=False):
    chunks, partials = shape_of(sizes)
    single = int((sizes <= CHUNK).sum())
    return {"k_ss_chunk_sums": 4.0 * L * C + 4.0 * L * (2 if weighted else 1) + 12.0 * S + 4.0 * C * (single + partials),
            "k_ss_segment_sums": 4.0 * C * partials + 4.0 * C * (S - single) + 8.0 * S,
            "k_vertex_gather (finish)": 8.0 * S * C}


def pool_faces_bytes(F, S, L, C, sizes):
    k = pool_bytes(F, S, L, C, sizes)
    del k["k_vertex_gather (finish)"]
    k["k_ss_gather_faces"] = 8.0 * F * C + 4.0 * F
    k["k_vertex_gather (finish, labels)"] = 4.0 * F * C + 4.0 * F
    return k


def block_labels(side=32, K=19):
    a, b = GRID
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    return np.repeat((((i // side) * 7 + (j // side) * 3) % K).astype(np.int32).reshape(-1), 2)


def host_route(source, seg):
    """`get()` (or the rows to the host), `ids()`, a numpy scatter-add; (seconds per step, sums)."""
    t0 = time.perf_counter()
    rows = source.get() if hasattr(source, "get") else source.numpy()
    ids = seg.ids()
    t1 = time.perf_counter()
    out = np.zeros((seg.count, rows.shape[1]), np.float32)
    sel = ids >= 0
    np.add.at(out, ids[sel], rows[sel])
    t2 = time.perf_counter()
    return dict(how="get() / numpy(), ids(), np.add.at", to_host_s=t1 - t0, scatter_add_s=t2 - t1, repeats=1), out


def main():
    kernels_only = "--kernels" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "segment_stats_bench.json")
    mesh = synth.grid_mesh(*GRID)
    F, V = len(mesh.faces), len(mesh.vertices)
    rng = np.random.default_rng(0)
    graph = fusion.FaceGraph.from_mesh(mesh)
    blocks = block_labels()
    noisy = blocks.copy()
    hit = rng.random(F) < 0.03
    noisy[hit] = rng.integers(0, 19, int(hit.sum()))
    legs = {"constant": np.full(F, 5, np.int32), "blocks": blocks, "blocks_3pct_noise": noisy}
    d_labels = {k: device.to_device(v) for k, v in legs.items()}

    def rows_of(C):
        rows = (rng.random((F, C), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
        rows[np.arange(F), noisy] += np.float32(1.0)
        rows /= rows.sum(axis=1, keepdims=True)
        rows[rng.random(F) < 0.1] = 0.0                               # faces no view observed
        return rows

    def aggregator_of(rows_h):
        agg = fusion.MeshAggregator(F, rows_h.shape[1])
        for lo in range(0, F, 250000):
            agg.set_raw_rows(lo, rows_h[lo:lo + 250000])
        return agg

    if kernels_only:
        d_rows = device.to_device(rows_of(19))
        for name in legs:
            seg = graph.segments(d_labels[name])
            seg.members_device()
            seg.pool_sums_device(d_rows)
            seg.pooled_face_labels_device(d_rows)
            seg.despeckle_labels_by_device(seg.sizes_device().numpy().astype(np.float32), 50.0)
        _lib.synchronize(0)
        return

    result = dict(tool="tools/segment_stats_bench.py", timing="host clock around smesh_synchronize; median of %d after a warm-up" % REPS,
                  faces=F, vertices=V,
                  sort_digit_rule="the one-bit stable split stays unless the %d-bit digit wins on the member-table leg by more than the "
                                  "repeats' min - max, in %d alternating pairs" % (WIDE_BITS, ROUNDS),
                  not_measured=["cfg5's 20 M faces", "real scans", "C >= 128", "sort digits of 2, 3 or more than 4 bits",
                                "meshes whose face order is not spatially coherent", "face weights"])

    def save():
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    segs = {}
    for name in legs:
        seg = segs[name] = graph.segments(d_labels[name])
        sizes = seg.sizes()
        S, L = seg.count, seg.num_labelled
        chunks, partials = shape_of(sizes)
        r = with_bytes(timed(lambda s: s.members_device(), setup=lambda: graph.segments(d_labels[name])), members_bytes(F, S, L))
        r.update(segments=S, largest=int(sizes.max()), chunks=chunks, partial_rows=partials)
        result["members_" + name] = r
        print("members", name, json.dumps(r, sort_keys=True), flush=True)
        rounds = []
        for _ in range(ROUNDS):                                       # alternating: one-bit, wide, one-bit, wide, ...
            pair = {}
            for bits in (1, WIDE_BITS):
                os.environ[SORT_ENV] = str(bits)
                pair["bits_%d" % bits] = timed(lambda s: s.members_device(), setup=lambda: graph.segments(d_labels[name]))
            rounds.append(pair)
        os.environ.pop(SORT_ENV, None)
        narrow, wide = "bits_1", "bits_%d" % WIDE_BITS
        result["sort_digit_" + name] = dict(rounds=rounds, wide_wins=bool(all(p[wide]["max_ms"] < p[narrow]["min_ms"] for p in rounds)))
        print("digit", name, json.dumps(result["sort_digit_" + name], sort_keys=True), flush=True)
        measure = device.to_device(sizes.astype(np.float32))
        r = with_bytes(timed(lambda: seg.despeckle_labels_by_device(measure, 50.0)), {"k_ss_despeckle_labels": 12.0 * F + 4.0 * S})
        result["despeckle_labels_by_" + name] = r
        print("despeckle", name, json.dumps(r, sort_keys=True), flush=True)
    save()
    for C in (19, 40):
        rows_h = rows_of(C)
        d_rows = device.to_device(rows_h)
        agg = aggregator_of(rows_h)
        for name in legs:
            seg = segs[name]
            sizes = seg.sizes()
            S, L = seg.count, seg.num_labelled
            r = {}
            for kind, source in (("rows", d_rows), ("aggregator", agg)):
                r["pool_sums_device_from_" + kind] = with_bytes(timed(lambda: seg.pool_sums_device(source)), pool_bytes(F, S, L, C, sizes))
                r["pooled_face_labels_device_from_" + kind] = with_bytes(timed(lambda: seg.pooled_face_labels_device(source)),
                                                                         pool_faces_bytes(F, S, L, C, sizes))
            result["C%d_%s" % (C, name)] = r
            print("C=%d" % C, name, json.dumps(r, sort_keys=True), flush=True)
            save()
        if C == 19:      # the route without this interface, once
            seg = segs["blocks_3pct_noise"]
            route, host = host_route(agg, seg)
            dev = seg.pool_sums(agg)
            scale = np.maximum(np.abs(dev), np.float32(1e-30))
            route["largest_relative_difference_observed"] = float((np.abs(host.astype(np.float64) - dev) / scale).max())
            route["note"] = "np.add.at adds in face order without chunks: another order of additions, so no parity is claimed"
            result["host_route_blocks_3pct_noise_C19"] = route
            print("host", route, flush=True)
        del agg, d_rows
        device.trim()
        save()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
