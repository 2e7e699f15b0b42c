"""Fused rows and areas pooled over segments (include/smesh_segment_stats.h, fusion.FaceGraph.face_areas, fusion.FaceSegments.pool*),
the part that needs no GPU: the extension header and its ctypes table, the restatement of the GPU tests (tests/segment_stats_ref.py)
against answers derived by hand, and the argument checks that come before anything is enqueued."""
import os
import re
import subprocess

import numpy as np
import pytest

import segment_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "smesh_segment_stats.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")

SYMBOLS = ["smesh_segment_stats_face_areas", "smesh_segment_stats_members", "smesh_segment_stats_pool", "smesh_segment_stats_pool_faces",
           "smesh_aggregator_segment_stats_pool", "smesh_aggregator_segment_stats_pool_faces", "smesh_segment_stats_despeckle_labels",
           "smesh_segment_stats_despeckle_rows", "smesh_aggregator_segment_stats_despeckle"]


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(HEADER)
    assert declared == sorted(SYMBOLS)
    assert all(n.startswith("smesh_segment_stats_") or n.startswith("smesh_aggregator_segment_stats_") for n in declared)
    assert declared == sorted(_lib.SEGMENT_STATS_SIGNATURES)       # every declared symbol has its ctypes signature
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    assert "smesh_face_segments_tables" not in open(HEADER).read()  # the segments' tables stay internal
    for other in sorted(os.listdir(INCLUDE)):                      # disjoint from smesh.h and every other header ...
        if other != "smesh_segment_stats.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    tables = [k for k in vars(_lib) if k.endswith("SIGNATURES") and k != "SEGMENT_STATS_SIGNATURES"]
    assert "SIGNATURES" in tables and "FACE_SEGMENTS_SIGNATURES" in tables and len(tables) >= 16
    for k in tables:                                               # ... and from every other table
        assert not set(declared) & set(getattr(_lib, k)), k


# ---- the restatement against answers derived by hand ---------------------------------------------------------------------------
def test_a_chain_of_three_faces():
    ids = np.array([0, 1, 0], np.int32)                            # faces 0 and 2 belong together, face 1 stands alone
    rows = np.array([[1, 2], [10, 20], [100, 200]], np.float32)
    offsets, members = ref.members(ids, 2)
    assert offsets.dtype == members.dtype == np.uint32
    assert (offsets.tolist(), members.tolist()) == ([0, 2, 3], [0, 2, 1])
    assert ref.pooled(rows, ids, 2).tolist() == [[101, 202], [10, 20]]
    assert ref.pooled_faces(rows, ids, 2).tolist() == [[101, 202], [10, 20], [101, 202]]
    ids = np.array([0, -1, 0], np.int32)                           # an unlabelled face keeps its own row, bit for bit
    rows[1] = [-0.0, 1e-42]
    x = ref.pooled_faces(rows, ids, 1, weights=np.array([2, 7, 3], np.float32))
    assert np.array_equal(u32(x), u32(np.array([[302, 604], [-0.0, 1e-42], [302, 604]], np.float32)))
    assert ref.members(np.full(3, -1), 0)[0].tolist() == [0] and len(ref.members(np.full(3, -1), 0)[1]) == 0
    assert ref.pooled(rows, np.full(3, -1), 0).shape == (0, 2)
    out, labels = ref.finish(np.array([[1, 3], [0.25, 0.25], [2, 2]], np.float32), ref.ANNOTATIONS, 0.9)
    assert out.tolist() == [[0.25, 0.75], [0, 0], [0.5, 0.5]] and labels.tolist() == [1, -1, 0]
    out, labels = ref.finish(np.array([[1, 3], [0.25, 0.25]], np.float32), ref.SUMS, 0.9)
    assert out.tolist() == [[1, 3], [0.25, 0.25]] and labels.tolist() == [1, -1]


def serial(values):
    acc = np.float32(0.0)
    for v in np.asarray(values, np.float32):
        acc = np.float32(acc + v)
    return acc


def test_chunks_of_256_change_the_bits_of_a_sum():
    """258 members: 256 of 65 536, then two of 1.  The serial sum stays at 2^24 (2^24 + 1 rounds back to even, twice); the rule adds
    the second chunk's 2 to the first chunk's 2^24 and gets 2^24 + 2.  (257 members cannot show it: a chunk of one member is the
    member, 0 + x = x, so the rule's sum IS the serial one -- asserted below -- and so is every sum of at most 256 members.)"""
    values = np.array([65536.0] * 256 + [1.0, 1.0], np.float32)
    ids = np.zeros(258, np.int32)
    got = ref.pooled(values[:, None], ids, 1)[0, 0]
    assert serial(values) == np.float32(2 ** 24) and got == np.float32(2 ** 24 + 2)
    assert u32(got) != u32(serial(values))
    rng = np.random.default_rng(257)
    for n in (1, 255, 256, 257):
        v = (rng.random(n, dtype=np.float32) * np.float32(2.0) ** rng.integers(-20, 21, n)).astype(np.float32)
        assert u32(ref.pooled(v[:, None], np.zeros(n, np.int32), 1)[0, 0]) == u32(serial(v))
    # the members of a segment are its faces in ascending order, wherever they lie: interleave the 258 with another segment
    ids2 = np.zeros(516, np.int32)
    ids2[1::2] = 1
    rows = np.zeros((516, 1), np.float32)
    rows[0::2, 0], rows[1::2, 0] = values, values[::-1]
    got2 = ref.pooled(rows, ids2, 2)[:, 0]
    assert got2[0] == np.float32(2 ** 24 + 2)
    # reversed: the chunk of 1, 1, 65 536 x 254 holds 2 + 254 * 2^16 exactly; the last two members make the second chunk, 2^17
    assert got2[1] == np.float32(2 + 256 * 65536)


def test_weights_are_one_multiplication_before_the_sum():
    rows = np.array([[3.0], [1e30], [5.0]], np.float32)
    w = np.array([0.1, 1e30, 2.0], np.float32)
    ids = np.array([0, 1, 0], np.int32)
    got = ref.pooled(rows, ids, 2, weights=w)
    want0 = np.float32(np.float32(0.0) + np.float32(np.float32(0.1) * np.float32(3.0))) + np.float32(10.0)
    assert u32(got[0, 0]) == u32(np.float32(want0)) and np.isinf(got[1, 0])      # (an overflow is what IEEE gives)
    assert ref.pooled(rows, ids, 2)[:, 0].tolist() == [8.0, np.float32(1e30)]


def test_face_areas_by_hand():
    vertices = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [6, 0, 0], [1, 1, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [4, 4, 4], [2, 1, 0]], np.int32)      # 3-4-5, collinear, a point, 3-4-5 turned over
    area = ref.face_areas(vertices, faces)
    assert area.dtype == np.float32 and area.tolist() == [6.0, 0.0, 0.0, 6.0]
    assert not u32(area[1:3]).any()                                # +0.0, every bit
    assert ref.areas(area, np.array([0, 0, -1, 1]), 2).tolist() == [6.0, 6.0]
    vertices[1, 0] = np.inf
    with np.errstate(all="ignore"):
        assert np.isnan(ref.face_areas(vertices, faces)[0])       # inf * 0: whatever IEEE gives


def test_despeckle_by_a_measure_and_a_nan():
    labels = np.array([2, -1, 2, 2, -7, 4], np.int32)
    ids = np.array([0, -1, 1, 1, -1, 2], np.int32)
    nan = float("nan")
    measure = np.array([0.5, nan, 2.0], np.float32)
    out, faces, segs = ref.despeckle_labels_by(labels, ids, measure, 0.5)         # >= : equality passes; the NaN segment goes
    assert out.tolist() == [2, -1, -1, -1, -1, 4] and (faces, segs) == (2, 1)
    out, faces, segs = ref.despeckle_labels_by(labels, ids, measure, 0.0)         # a NaN fails even a minimum of 0
    assert out.tolist() == [2, -1, -1, -1, -1, 4] and (faces, segs) == (2, 1)
    out, faces, segs = ref.despeckle_labels_by(labels, ids, measure, 1.0)
    assert out.tolist() == [-1, -1, -1, -1, -1, 4] and (faces, segs) == (3, 2)
    out, faces, segs = ref.despeckle_labels_by(labels, ids, measure, nan)         # a NaN minimum removes everything
    assert out.tolist() == [-1] * 6 and (faces, segs) == (4, 3)
    out, faces, segs = ref.despeckle_labels_by(labels, ids, np.array([1, 1, 1], np.float32), 0.0)
    assert out.tolist() == [2, -1, 2, 2, -1, 4] and (faces, segs) == (0, 0)
    rows = np.array([[0.5, 0.5], [-0.0, 1e-42], [1, 0], [0, 1], [0.25, -0.0], [7, 7]], np.float32)
    got = ref.despeckle_rows_by(rows, ids, measure, 0.5)
    want = rows.copy()
    want[2:4] = 0.0
    assert got.dtype == np.float32 and np.array_equal(u32(got), u32(want))      # -0.0 and a subnormal pass through


# ---- argument checks that need no device ---------------------------------------------------------------------------------------
def test_wrong_arguments_are_refused_before_a_device_is_needed():
    from semantic_meshes_amd import fusion
    g = object.__new__(fusion.FaceGraph)                              # a graph that was never built: the checks come first
    g.num_faces, g.num_vertices, g.num_entries, g.device, g._h = 4, 6, 6, 0, None
    for bad in (np.zeros((6, 3), np.float64), np.zeros((5, 3), np.float32), np.zeros((6, 2), np.float32), np.zeros(18, np.float32)):
        with pytest.raises(ValueError):
            g.face_areas(bad)
        with pytest.raises(ValueError):
            g.face_areas_device(bad)
    s = object.__new__(fusion.FaceSegments)                           # segments that were never made
    s._h, s.device, s.num_faces, s.count, s.num_labelled = None, 0, 4, 2, 4
    rows, w, measure = np.zeros((4, 3), np.float32), np.ones(4, np.float32), np.ones(2, np.float32)
    pools = (s.pool_sums, s.pool, s.pool_labels, s.pool_sums_device, s.pool_device, s.pool_labels_device, s.pooled_face_sums,
             s.pooled_face_annotations, s.pooled_face_labels, s.pooled_face_sums_device, s.pooled_face_annotations_device,
             s.pooled_face_labels_device)
    for call in pools:
        for bad in (np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32), np.zeros((4, 0), np.float32)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in (np.ones(4, np.float64), np.ones(3, np.float32), np.ones(5, np.float32), np.ones((4, 1), np.float32), np.ones(4, np.int32)):
            with pytest.raises(ValueError):
                call(rows, face_weights=bad)
    for bad in (None, np.ones(4, np.float64), np.ones(3, np.float32), np.ones((4, 1), np.float32)):
        with pytest.raises(ValueError):
            s.areas(bad)
        with pytest.raises(ValueError):
            s.areas_device(bad)
    for bad in ("0.5", None, True, [0.5]):                            # a minimum that is no number
        with pytest.raises(ValueError):
            s.despeckle_labels_by(measure, bad)
        with pytest.raises(ValueError):
            s.despeckle_labels_by_device(measure, bad, return_removed=True)
        with pytest.raises(ValueError):
            s.despeckle_sums_by(rows, measure, bad)
        with pytest.raises(ValueError):
            s.despeckle_sums_by_device(rows, measure, bad)
    for bad in (None, np.ones(2, np.float64), np.ones(3, np.float32), np.ones(1, np.float32), np.ones((2, 1), np.float32), np.ones(2, np.int32)):
        with pytest.raises(ValueError):
            s.despeckle_labels_by(bad, 0.5)
        with pytest.raises(ValueError):
            s.despeckle_sums_by(rows, bad, 0.5)
    for bad in (np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32)):
        with pytest.raises(ValueError):
            s.despeckle_sums_by(bad, measure, 0.5)
