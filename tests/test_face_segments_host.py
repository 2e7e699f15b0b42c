"""Segments of a labelled mesh (include/smesh_face_segments.h, fusion.FaceGraph.segments, fusion.FaceSegments), the part that needs no
GPU: the extension header and its ctypes table, the flood-fill restatement of the GPU tests (tests/face_segments_ref.py) against
answers derived by hand, and the argument checks that come before anything is enqueued."""
import os
import re
import subprocess

import numpy as np
import pytest

import face_graph_ref as gref
import face_segments_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "smesh_face_segments.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")

SYMBOLS = ["smesh_face_segments_create", "smesh_aggregator_face_segments", "smesh_face_segments_destroy", "smesh_face_segments_size",
           "smesh_face_segments_get", "smesh_face_segments_despeckle_labels", "smesh_face_segments_despeckle_rows",
           "smesh_aggregator_face_segments_despeckle"]


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(HEADER)
    assert declared == sorted(SYMBOLS)
    assert all(n.startswith("smesh_face_segments_") or n.startswith("smesh_aggregator_face_segments") for n in declared)
    assert declared == sorted(_lib.FACE_SEGMENTS_SIGNATURES)       # every declared symbol has its ctypes signature
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    assert "smesh_face_graph_tables" not in open(HEADER).read()    # the graph's tables stay internal
    for other in sorted(os.listdir(INCLUDE)):                      # disjoint from smesh.h and every other header ...
        if other != "smesh_face_segments.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    tables = [k for k in vars(_lib) if k.endswith("SIGNATURES") and k != "FACE_SEGMENTS_SIGNATURES"]
    assert "SIGNATURES" in tables and "FACE_GRAPH_SIGNATURES" in tables and len(tables) >= 15
    for k in tables:                                               # ... and from every other table
        assert not set(declared) & set(getattr(_lib, k)), k


# ---- the restatement against answers derived by hand ---------------------------------------------------------------------------
def seg(faces, V, labels, weights=None, min_weight=None):
    off, nbr = gref.adjacency(np.asarray(faces, np.int32).reshape(-1, 3), V)
    ids, first, label, size = ref.segments(off, nbr, np.asarray(labels), None if weights is None else np.asarray(weights, np.float32), min_weight)
    assert ids.dtype == np.int32 and first.dtype == np.uint32 and label.dtype == np.int32 and size.dtype == np.uint32
    assert len(first) == len(label) == len(size) and int(size.sum()) == int((np.asarray(labels) >= 0).sum())
    return ids.tolist(), first.tolist(), label.tolist(), size.tolist()


TWO = [[0, 1, 2], [1, 3, 2]]
STRIP5 = [[k, k + 1, k + 2] for k in range(5)]       # a chain: face k touches k - 1 and k + 1


def test_two_triangles_sharing_an_edge():
    assert seg(TWO, 4, [3, 3]) == ([0, 0], [0], [3], [2])
    assert seg(TWO, 4, [3, 4]) == ([0, 1], [0, 1], [3, 4], [1, 1])
    assert seg(TWO, 4, [0, 0]) == ([0, 0], [0], [0], [2])                           # label 0 is a label
    big = 2 ** 31 - 1
    assert seg(TWO, 4, np.array([big, big], np.int32)) == ([0, 0], [0], [big], [2])


def test_a_fan_around_a_vertex_does_not_link():
    assert seg([[0, 1, 2], [0, 3, 4], [0, 5, 6]], 7, [1, 1, 1]) == ([0, 1, 2], [0, 1, 2], [1, 1, 1], [1, 1, 1])      # only edges link


def test_a_duplicate_face_and_a_non_manifold_edge():
    dup = [[0, 1, 2], [0, 1, 2], [1, 3, 2]]
    assert seg(dup, 4, [1, 1, 1]) == ([0, 0, 0], [0], [1], [3])
    assert seg(dup, 4, [1, 2, 1]) == ([0, 1, 0], [0, 1], [1, 2], [2, 1])            # faces 0 and 2 share the edge {1, 2}
    four = [[0, 1, 2], [0, 1, 3], [0, 1, 4], [1, 0, 5]]                             # one edge in four faces: everyone lists everyone
    assert seg(four, 6, [5, 6, 5, 6]) == ([0, 1, 0, 1], [0, 1], [5, 6], [2, 2])
    assert seg(four, 6, [5, 5, 5, 5]) == ([0, 0, 0, 0], [0], [5], [4])


def test_negative_labels_belong_to_no_segment():
    # -7 next to -7: equal, but not labelled; -1 between two faces of label 2 separates them
    assert seg(STRIP5, 7, [2, -1, 2, -7, -7]) == ([0, -1, 1, -1, -1], [0, 2], [2, 2], [1, 1])
    assert seg(STRIP5, 7, [-1] * 5) == ([-1] * 5, [], [], [])
    # numbering follows the lowest face: the segment of label 9 starts at face 0, that of label 4 at face 1
    assert seg(STRIP5, 7, [9, 4, 4, 9, 9]) == ([0, 1, 1, 2, 2], [0, 1, 3], [9, 4, 9], [1, 2, 2])


def test_weights_link_in_either_direction_and_a_nan_never_links():
    off, nbr = gref.adjacency(np.asarray(TWO), 4)
    assert nbr.tolist() == [1, 0]                                                   # entry 0: face 0 -> 1; entry 1: face 1 -> 0
    one, two = ([0, 0], [0], [7], [2]), ([0, 1], [0, 1], [7, 7], [1, 1])
    assert seg(TWO, 4, [7, 7], [1.0, 1.0], 0.5) == one
    assert seg(TWO, 4, [7, 7], [1.0, 0.0], 0.5) == one                              # w[f->g] passes, w[g->f] fails: linked
    assert seg(TWO, 4, [7, 7], [0.0, 1.0], 0.5) == one
    assert seg(TWO, 4, [7, 7], [0.0, 0.25], 0.5) == two
    assert seg(TWO, 4, [7, 7], [0.5, 0.0], 0.5) == one                              # >= : equality passes
    nan = float("nan")
    assert seg(TWO, 4, [7, 7], [nan, nan], 0.0) == two                              # a NaN weight does not link
    assert seg(TWO, 4, [7, 7], [nan, 1.0], 0.5) == one                              # ... but the other direction may
    assert seg(TWO, 4, [7, 7], [1.0, 1.0], nan) == two
    assert seg(TWO, 4, [7, 8], [1.0, 1.0], 0.5) == ([0, 1], [0, 1], [7, 8], [1, 1])  # weights never join different labels


def test_despeckle_by_hand():
    labels = np.array([2, -1, 2, 2, -7], np.int32)
    off, nbr = gref.adjacency(np.asarray(STRIP5), 7)
    ids, first, label, size = ref.segments(off, nbr, labels)
    assert (ids.tolist(), size.tolist()) == ([0, -1, 1, 1, -1], [1, 2])
    for min_faces in (0, 1):                                                        # nothing is removed
        out, faces, segs = ref.despeckle_labels(labels, ids, size, min_faces)
        assert out.tolist() == [2, -1, 2, 2, -1] and (faces, segs) == (0, 0)
    out, faces, segs = ref.despeckle_labels(labels, ids, size, 2)
    assert out.tolist() == [-1, -1, 2, 2, -1] and (faces, segs) == (1, 1)
    out, faces, segs = ref.despeckle_labels(labels, ids, size, 3)
    assert out.tolist() == [-1] * 5 and (faces, segs) == (3, 2)
    rows = np.array([[0.5, 0.5], [-0.0, 1e-42], [1, 0], [0, 1], [0.25, -0.0]], np.float32)
    got = ref.despeckle_rows(rows, labels, ids, size, 2)
    want = rows.copy()
    want[0] = 0.0
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))      # -0.0 and a subnormal pass through
    assert np.array_equal(ref.despeckle_rows(rows, labels, ids, size, 1).view(np.uint32), rows.view(np.uint32))
    assert not ref.despeckle_rows(rows, labels, ids, size, 3)[[0, 2, 3]].view(np.uint32).any()        # +0.0, every bit


def test_no_faces_and_labels_from_rows():
    off, nbr = gref.adjacency(np.zeros((0, 3), np.int32), 0)
    ids, first, label, size = ref.segments(off, nbr, np.zeros(0, np.int32))
    assert (len(ids), len(first), len(label), len(size)) == (0, 0, 0, 0)
    out, faces, segs = ref.despeckle_labels(np.zeros(0, np.int32), ids, size, 5)
    assert len(out) == 0 and (faces, segs) == (0, 0)
    rows = np.array([[0.2, 0.7, 0.1], [0.5, 0.5, 0.0], [0.1, 0.2, 0.1], [0, 0, 0]], np.float32)
    assert ref.row_labels(rows, 0.9).tolist() == [1, 0, -1, -1]                     # argmax, the lowest class on a tie, -1 below 0.9


# ---- argument checks that need no device ---------------------------------------------------------------------------------------
def test_wrong_arguments_are_refused_before_a_device_is_needed():
    from semantic_meshes_amd import fusion
    g = object.__new__(fusion.FaceGraph)                              # a graph that was never built: the checks come first
    g.num_faces, g.num_vertices, g.num_entries, g.device, g._h = 4, 6, 6, 0, None
    labels, w = np.zeros(4, np.int32), np.ones(6, np.float32)
    for bad in (np.zeros(4, np.float32), np.zeros(4, np.float64), np.zeros(4, bool), np.zeros(5, np.int32), np.zeros(3, np.int64),
                np.zeros((4, 1, 1), np.int32), np.full(4, 2 ** 31, np.int64), np.zeros((4, 3), np.int32), np.zeros((4, 3), np.float64)):
        with pytest.raises(ValueError):
            g.segments(bad)
    with pytest.raises(ValueError):
        g.segments(labels, weights=w)                                 # weights without min_weight
    with pytest.raises(ValueError):
        g.segments(labels, min_weight=0.5)                            # min_weight without weights
    for bad in ("0.5", True, [0.5]):
        with pytest.raises(ValueError):
            g.segments(labels, weights=w, min_weight=bad)
    for bad in (np.ones(6, np.float64), np.ones(5, np.float32), np.ones(7, np.float32), np.ones((6, 1), np.float32), np.ones(6, np.int32)):
        with pytest.raises(ValueError):
            g.segments(labels, weights=bad, min_weight=0.5)
    s = object.__new__(fusion.FaceSegments)                           # segments that were never made
    s._h, s.device, s.num_faces, s.count, s.num_labelled = None, 0, 4, 0, 0
    rows = np.zeros((4, 3), np.float32)
    for bad in (-1, 1.5, "3", None, True, 2 ** 32):
        with pytest.raises(ValueError):
            s.despeckle_labels(bad)
        with pytest.raises(ValueError):
            s.despeckle_labels_device(bad, return_removed=True)
        with pytest.raises(ValueError):
            s.despeckle_sums(rows, bad)
        with pytest.raises(ValueError):
            s.despeckle_sums_device(rows, bad)
    for bad in (np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32), np.zeros((4, 0), np.float32)):
        with pytest.raises(ValueError):
            s.despeckle_sums(bad, 3)
