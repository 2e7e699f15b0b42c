"""The mesh-graph kernels past the sizes at which their launches change, against the numpy references (tests/face_graph_ref.py,
tests/face_segments_ref.py, tests/points_ref.py) on the cases of tests/mesh_graph_scale_cases.py.  The sibling modules stop at
30 000 faces; the product's meshes have a million.  What only a mesh of this size executes:

  * k_scan_sums' second chunk and its carry (scan.inc.hpp, compiled separately into face_graph.hip, face_segments.hip, points.hip and
    vertices.hip): a scan of more than 256 * 1024 elements;
  * the second turn of the strided loops of k_seg_flatten, k_seg_despeckle_labels and k_seg_small (face_segments.hip): more than
    2048 * 256 items, for k_seg_small that many SEGMENTS;
  * the union-find under thousands of workgroups that arrive in turns, on a spatially coherent face order and on a shuffled one;
  * every k_face_propagate<G, NCH> and k_vertex_gather<64, NCH> that launch_propagate / launch_gather can pick.

Every result here is defined to the bit, so every comparison is exact (floats as their uint32 patterns), and every expected value is
computed on the host.  Error paths and the checks that inputs stay unchanged are the sibling modules' (tests/test_gpu_face_graph.py,
tests/test_gpu_face_segments.py, tests/test_gpu_points.py, tests/test_gpu_vertices.py).

Durations on an MI355X (DURATIONS below, `pytest --durations`, one run, each reference computed by the first test that needs it): the
whole module, 42 tests, 9.2 s; the slowest test 1.03 s (the point index: the exhaustive reference of 16 points over 530 000 faces); a
segments case on the big grid 0.4 - 0.8 s, a graph build 0.04 - 0.3 s, a k_face_propagate instance 0.02 s or less.
"""
import numpy as np
import pytest

import face_graph_ref as gref
import face_segments_ref as sref
import mesh_graph_scale_cases as cases
import test_gpu_face_graph as tgf
import test_gpu_face_segments as tfs
import test_gpu_points as tp
import test_gpu_vertices as tv

pytestmark = pytest.mark.gpu

THRESHOLD = cases.THRESHOLD

# Measured on an MI355X (seconds): the whole module and the slowest test of each part.
DURATIONS = {
    "module": 9.2,
    "test_the_point_index_scans_more_cells_than_one_chunk": 1.03,
    "test_segments_equal_the_flood_fill[shuffled-constant]": 0.80,
    "test_weighted_smoothing_on_the_big_grid_is_bit_equal": 0.77,
    "test_weighted_segments_equal_the_flood_fill[constant-normal]": 0.53,
    "test_fill_on_the_big_grid_is_bit_equal": 0.35,
    "test_the_graph_equals_the_restatement[shuffled]": 0.30,
    "test_more_segments_than_the_capped_grid_has_lanes[constant]": 0.22,
    "test_segments_at_the_edge_sizes[524287]": 0.21,
    "test_every_propagate_instance_is_bit_equal[512]": 0.02,
}


def first_difference(got, want):
    """For a failure's message: the first element at which two arrays differ."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s and %s" % (got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(-1))
    if not len(bad):
        return "equal"
    k = np.unravel_index(int(bad[0]), got.shape)
    return "%d of %d differ, first at %s: got %r, want %r" % (len(bad), got.size, k, got[k], want[k])


def assert_equal(got, want, what):
    assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))


# ---- a. the graph at every size --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.GRAPH_CASES)
def test_the_graph_equals_the_restatement(sm, name):
    faces, vertices, V, want_off, want_nbr = cases.case(name)
    graph = sm.fusion.FaceGraph(faces, V)
    assert (graph.num_faces, graph.num_vertices, graph.num_entries) == (len(faces), V, len(want_nbr))
    offsets, nbr = graph.adjacency()
    assert offsets.dtype == np.uint64 and nbr.dtype == np.uint32
    assert_equal(offsets, want_off, "%s offsets" % name)
    assert_equal(nbr, want_nbr, "%s neighbours" % name)


@pytest.mark.parametrize("V", cases.VERTEX_COUNTS)
def test_the_vertex_map_across_the_scan_chunk(sm, V):
    faces, nv = cases.vertex_case(V)
    offsets, adj = sm.fusion.VertexTransfer(faces, nv).adjacency()
    want_off, want_adj = tv.np_csr(faces, nv)
    assert_equal(offsets, want_off, "V = %d offsets" % V)
    assert_equal(adj, want_adj, "V = %d faces" % V)


# ---- b. segments on the big grid -------------------------------------------------------------------------------------------------
def graph_of(sm, name):
    faces, vertices, V, offsets, nbr = cases.case(name)
    return sm.fusion.FaceGraph(faces, V)


def assert_segments_equal(a, b):
    for what in ("ids", "first_faces", "labels", "sizes"):
        assert_equal(getattr(a, what)(), getattr(b, what)(), "a second call's " + what)
    assert (a.count, a.num_labelled) == (b.count, b.num_labelled)


@pytest.mark.parametrize("name,pattern", [("big", p) for p in cases.BIG_PATTERNS] + [("shuffled", "constant"), ("shuffled", "blocks32_noisy")])
def test_segments_equal_the_flood_fill(sm, name, pattern):
    from semantic_meshes_amd.device import to_device
    labels, want = cases.labels(name, pattern), cases.expected(name, pattern)
    graph = graph_of(sm, name)
    d_labels = to_device(labels)
    first = graph.segments(d_labels)
    assert_equal(first.ids(), want[0], "%s %s ids" % (name, pattern))
    tfs.check_segments(first, labels, want, min_faces_list=(0, 50), class_counts=(19,), seed=len(pattern))
    assert_segments_equal(graph.segments(d_labels), first)


@pytest.mark.parametrize("pattern,kind", [("constant", "normal"), ("blocks32_noisy", "asymmetric")])
def test_weighted_segments_equal_the_flood_fill(sm, pattern, kind):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = cases.case("big")
    labels, want = cases.labels("big", pattern), cases.expected("big", pattern, kind)
    w, min_weight = cases.entry_weights("big", kind)
    graph = graph_of(sm, "big")
    d_w = graph.normal_weights(vertices) if kind == "normal" else to_device(w)
    assert_equal(tfs.u32(d_w.numpy()), tfs.u32(w), "weights")
    d_labels = to_device(labels)
    first = graph.segments(d_labels, weights=d_w, min_weight=min_weight)
    assert_equal(first.ids(), want[0], "%s %s ids" % (pattern, kind))
    tfs.check_segments(first, labels, want, min_faces_list=(0, 50), class_counts=(19,), seed=3)
    assert_segments_equal(graph.segments(d_labels, weights=d_w, min_weight=min_weight), first)


# ---- c. segments at the four edge sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", cases.EDGE_FACES)
def test_segments_at_the_edge_sizes(sm, F):
    from semantic_meshes_amd.device import to_device
    name = "first%d" % F
    labels = cases.labels(name, "random2")
    ids, first, label, size = cases.expected(name, "random2")
    seg = graph_of(sm, name).segments(to_device(labels))
    assert (seg.num_faces, seg.count, seg.num_labelled) == (F, len(first), int((labels >= 0).sum()))
    assert_equal(seg.ids(), ids, "F = %d ids" % F)
    assert_equal(seg.first_faces(), first, "F = %d first faces" % F)
    assert_equal(seg.labels(), label, "F = %d labels" % F)
    assert_equal(seg.sizes(), size, "F = %d sizes" % F)
    out, faces_gone, segs_gone = sref.despeckle_labels(labels, ids, size, 3)
    got, n1, n2 = seg.despeckle_labels(3, return_removed=True)
    assert_equal(got, out, "F = %d despeckled labels" % F)
    assert (n1, n2) == (faces_gone, segs_gone) and faces_gone > 0 and 0 < segs_gone < len(first)


# ---- d. more segments than the capped grid has lanes -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["constant", "seventh"])
def test_more_segments_than_the_capped_grid_has_lanes(sm, pattern):
    from semantic_meshes_amd.device import to_device
    labels = cases.labels("isolated", pattern)
    ids, first, label, size = cases.expected("isolated", pattern)
    num_labelled = int((labels >= 0).sum())
    assert len(first) == num_labelled and (num_labelled > cases.CAPPED_GRID) == (pattern == "constant")      # (seventh: 454 285)
    seg = graph_of(sm, "isolated").segments(to_device(labels))
    assert (seg.num_faces, seg.count, seg.num_labelled) == (len(labels), num_labelled, num_labelled)
    assert_equal(seg.ids(), np.where(labels >= 0, np.cumsum(labels >= 0) - 1, -1).astype(np.int32), "ids as a running count")
    assert_equal(seg.ids(), ids, "ids")
    assert_equal(seg.first_faces(), first, "first faces")
    assert_equal(seg.sizes(), np.ones(num_labelled, np.uint32), "sizes")
    got, n1, n2 = seg.despeckle_labels(2, return_removed=True)
    assert_equal(got, np.full(len(labels), -1, np.int32), "despeckled labels")
    assert (n1, n2) == (num_labelled, num_labelled) == sref.despeckle_labels(labels, ids, size, 2)[1:]      # (n2: k_seg_small's strided turn)
    got, n1, n2 = seg.despeckle_labels(1, return_removed=True)
    assert_equal(got, np.where(labels >= 0, labels, -1).astype(np.int32), "labels kept")
    assert (n1, n2) == (0, 0)


# ---- e. propagation at size --------------------------------------------------------------------------------------------------------
def test_fill_on_the_big_grid_is_bit_equal(sm):
    from semantic_meshes_amd.device import to_device
    rows, _, want, tot = cases.propagated(gref.FILL)
    labels, dc, unreached = gref.finish(want, tot, THRESHOLD)
    graph = graph_of(sm, "big")
    d_rows = to_device(rows)
    sums, n1 = graph.fill_sums(d_rows, 2, THRESHOLD, None, return_unreached=True)
    assert_equal(tgf.bits(sums), tgf.bits(want), "fill sums (bits)")
    got_labels, n2 = graph.fill_labels(d_rows, 2, THRESHOLD, None, THRESHOLD, return_unreached=True)
    assert got_labels.dtype == np.int32
    assert_equal(got_labels, labels, "fill labels")
    assert (n1, n2) == (unreached, unreached)
    assert (labels == -1).any() and (labels >= 0).mean() > 0.8


def test_weighted_smoothing_on_the_big_grid_is_bit_equal(sm):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = cases.case("big")
    rows, w, want, tot = cases.propagated(gref.SMOOTH)
    labels, dc, unreached = gref.finish(want, tot, THRESHOLD)
    graph = graph_of(sm, "big")
    d_w = graph.normal_weights(vertices)
    assert_equal(tgf.bits(d_w.numpy()), tgf.bits(w), "normal weights (bits)")
    d_rows = to_device(rows)
    sums, n1 = graph.smooth_sums(d_rows, 2, 0.5, d_w, return_unreached=True)
    assert_equal(tgf.bits(sums), tgf.bits(want), "smooth sums (bits)")
    got_labels, n2 = graph.smooth_labels(d_rows, 2, 0.5, d_w, THRESHOLD, return_unreached=True)
    assert got_labels.dtype == np.int32
    assert_equal(got_labels, labels, "smooth labels")
    assert (n1, n2) == (unreached, unreached)


# ---- f. every k_face_propagate instance --------------------------------------------------------------------------------------------
# launch_propagate (face_graph.hip), from the comment above it: one lane for one class, two for two; groups of 4 lanes up to 32
# classes and of 8 lanes up to 64, a wave beyond; the lanes of a group hold NCH = ceil(C / G) classes each -- an 8-lane group at
# least 5, since four or fewer per lane is a 4-lane group's row -- up to 8; beyond 512 classes the chunk-after-chunk form, NCH = 0.
# Written down here, never read back from the library.
INSTANCE = {1: (1, 1), 2: (2, 1), 3: (4, 1), 4: (4, 1), 5: (4, 2), 9: (4, 3), 13: (4, 4), 19: (4, 5), 21: (4, 6), 25: (4, 7), 32: (4, 8),
            33: (8, 5), 40: (8, 5), 41: (8, 6), 49: (8, 7), 64: (8, 8),
            65: (64, 2), 150: (64, 3), 193: (64, 4), 257: (64, 5), 321: (64, 6), 385: (64, 7), 449: (64, 8), 512: (64, 8), 513: (64, 0)}
# every instantiation in launch_propagate's switches: 2 + 8 + 4 + 7 + 1
COMPILED = {(1, 1), (2, 1)} | {(4, n) for n in range(1, 9)} | {(8, n) for n in range(5, 9)} | {(64, n) for n in range(2, 9)} | {(64, 0)}
MORE_CLASS_COUNTS = [2, 3, 4, 9, 13, 21, 25, 41, 49, 193, 257, 321, 385, 449, 512]      # beside test_gpu_face_graph.CLASS_COUNTS


def instance_by_rule(C):
    if C <= 2:
        return (C, 1)
    if C <= 32:
        return (4, -(-C // 4))
    if C <= 64:
        return (8, max(5, -(-C // 8)))
    return (64, -(-C // 64) if C <= 512 else 0)


def test_the_expected_table_covers_every_instance():
    assert sorted(INSTANCE) == sorted(MORE_CLASS_COUNTS + tgf.CLASS_COUNTS) and not set(MORE_CLASS_COUNTS) & set(tgf.CLASS_COUNTS)
    assert all(INSTANCE[C] == instance_by_rule(C) for C in INSTANCE)
    assert len(COMPILED) == 22 and set(INSTANCE.values()) == COMPILED
    # what this module adds to the instances that test_gpu_face_graph.py launches
    before = {INSTANCE[C] for C in tgf.CLASS_COUNTS}
    assert {INSTANCE[C] for C in MORE_CLASS_COUNTS} - before == COMPILED - before and len(COMPILED - before) == 13


@pytest.mark.parametrize("C", MORE_CLASS_COUNTS)
def test_every_propagate_instance_is_bit_equal(sm, C):
    tgf.check_propagation(sm, tgf.grid_case(), C, 800 + C, [(gref.SMOOTH, 0.5, True)], [2], [False] * 4)


# ---- g. the point index's scan -----------------------------------------------------------------------------------------------------
def test_the_point_index_scans_more_cells_than_one_chunk(sm):
    from semantic_meshes_amd.device import to_device
    faces, vertices = cases.big_mesh()
    points, want = cases.near_points()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    st = index.stats()
    print("big grid:", st)
    assert st["faces"] == len(faces) and int(np.prod(st["dims"], dtype=np.int64)) + 1 > cases.SCAN_CHUNK
    assert (want[0] >= 0).all() and float(want[1].max()) <= 0.01 ** 2 * 1.01
    tp.assert_same(index.nearest(to_device(points)), want)
