"""Mesh-graph operations (include/smesh_face_graph.h, fusion.FaceGraph), the part that needs no GPU: the extension header and its
ctypes table, the numpy restatement of the GPU tests (tests/face_graph_ref.py) against answers derived by hand, and the argument
checks that come before anything is enqueued."""
import os
import re
import subprocess

import numpy as np
import pytest

import face_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FG_HEADER = os.path.join(INCLUDE, "smesh_face_graph.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", FG_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(FG_HEADER)
    assert declared == sorted(["smesh_face_graph_create", "smesh_face_graph_destroy", "smesh_face_graph_size", "smesh_face_graph_adjacency",
                               "smesh_face_graph_propagate", "smesh_aggregator_face_propagate", "smesh_face_graph_normal_weights"])
    assert declared == sorted(_lib.FACE_GRAPH_SIGNATURES)          # every declared symbol has its ctypes signature
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    for other in sorted(os.listdir(INCLUDE)):                      # disjoint from smesh.h and every other header ...
        if other != "smesh_face_graph.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    tables = [k for k in vars(_lib) if k.endswith("SIGNATURES") and k != "FACE_GRAPH_SIGNATURES"]
    assert "SIGNATURES" in tables and len(tables) >= 14
    for k in tables:                                               # ... and from every other table
        assert not set(declared) & set(getattr(_lib, k)), k


def test_mode_constants_agree_with_the_header():
    from semantic_meshes_amd import _lib
    defines = dict(re.findall(r"#\s*define\s+(SMESH_FG_[A-Z_]+)\s+(\d+)", open(FG_HEADER).read()))
    assert defines == {"SMESH_FG_SMOOTH": "0", "SMESH_FG_FILL": "1", "SMESH_FG_MAX_POWER": "16"}
    assert (_lib.FG_SMOOTH, _lib.FG_FILL, _lib.FG_MAX_POWER) == (0, 1, 16)
    assert (ref.SMOOTH, ref.FILL) == (_lib.FG_SMOOTH, _lib.FG_FILL)


# ---- the restatement against answers derived by hand ---------------------------------------------------------------------------
def lists(faces, V):
    off, nbr = ref.adjacency(np.asarray(faces, np.int32).reshape(-1, 3), V)
    assert off.dtype == np.uint64 and nbr.dtype == np.uint32 and off[0] == 0 and off[-1] == len(nbr)
    return [nbr[int(off[f]):int(off[f + 1])].tolist() for f in range(len(off) - 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_two_triangles_sharing_an_edge():
    faces = [[0, 1, 2], [1, 3, 2]]
    assert lists(faces, 4) == [[1], [0]]
    off, nbr = ref.adjacency(np.asarray(faces), 4)
    x0 = np.array([[1, 0], [0, 1]], np.float32)
    x, tot = ref.propagate(off, nbr, x0, 1, ref.SMOOTH, alpha=0.5)
    assert x.dtype == np.float32 and x.tolist() == [[0.5, 0.5], [0.5, 0.5]] and tot.tolist() == [1.0, 1.0]
    assert ref.propagate(off, nbr, x0, 0, ref.SMOOTH)[0].tolist() == x0.tolist()          # T = 0
    assert ref.propagate(off, nbr, x0, 3, ref.SMOOTH, alpha=0.0)[0].tolist() == x0.tolist()
    assert ref.propagate(off, nbr, x0, 1, ref.SMOOTH, alpha=1.0)[0].tolist() == [[0, 1], [1, 0]]
    # weights: a zero weight on the only entry of face 0 leaves it without informed weight (d == 0): it keeps x0
    x, _ = ref.propagate(off, nbr, x0, 1, ref.SMOOTH, alpha=0.5, weights=np.array([0, 2], np.float32))
    assert x.tolist() == [[1, 0], [0.5, 0.5]]


def test_a_closed_tetrahedron():
    assert lists([[0, 1, 2], [0, 1, 3], [2, 1, 3], [2, 0, 3]], 4) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    # the list follows the face's own slots: another winding of face 1 gives the same faces in another order
    assert lists([[0, 1, 2], [0, 3, 1], [2, 1, 3], [2, 0, 3]], 4)[1] == [3, 2, 0]


def test_fill_advances_one_ring_per_iteration_along_a_strip():
    n = 9
    faces = np.array([[k, k + 1, k + 2] for k in range(n)], np.int32)
    assert lists(faces, n + 2) == [[1]] + [[k - 1, k + 1] for k in range(1, n - 1)] + [[n - 2]]
    off, nbr = ref.adjacency(faces, n + 2)
    x0 = np.zeros((n, 2), np.float32)
    x0[0] = (0.3, 0.7)
    for T in range(n + 2):
        x, tot = ref.propagate(off, nbr, x0, T, ref.FILL, observed_threshold=0.9)
        reached = min(T, n - 1)
        assert np.array_equal(bits(x[:reached + 1]), np.tile(bits(x0[0]), (reached + 1, 1)))      # the observed row, bit for bit
        assert not x[reached + 1:].any()
        assert ref.finish(x, tot, 0.9)[2] == n - 1 - reached                                      # unreached counts down by one
        assert ref.finish(x, tot, 0.9)[0].tolist() == [1] * (reached + 1) + [-1] * (n - 1 - reached)


def test_repeated_vertices_duplicate_faces_and_a_non_manifold_edge():
    assert lists([[0, 1, 1], [0, 1, 2]], 3) == [[1], [0]]             # slots {1,1} and {1,0} of face 0 are skipped
    assert lists([[1, 1, 1], [0, 1, 2]], 3) == [[], []]
    assert lists([[0, 0, 1], [1, 0, 2]], 3) == [[1], [0]]             # slot 0 skipped, slot 2 repeats slot 1
    # the same face listed twice: each names the other once per shared edge
    assert lists([[0, 1, 2], [0, 1, 2], [1, 3, 2]], 4) == [[1, 1, 2, 1], [0, 0, 2, 0], [0, 1]]
    # one edge shared by four faces: every one lists the other three, ascending
    assert lists([[0, 1, 2], [0, 1, 3], [0, 1, 4], [1, 0, 5]], 6) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert lists(np.zeros((0, 3), np.int32), 0) == [] and lists([[0, 1, 2]], 3) == [[]]


def test_an_isolated_face_keeps_its_row_in_both_modes():
    off, nbr = ref.adjacency(np.array([[0, 1, 2], [3, 4, 5], [3, 4, 6]]), 7)
    x0 = np.array([[0.1, 0.2], [0, 0], [0.5, 0.5]], np.float32)
    for mode in (ref.SMOOTH, ref.FILL):
        trace = []
        x, tot = ref.propagate(off, nbr, x0, 2, mode, alpha=0.5, observed_threshold=0.9, trace=trace)
        assert np.array_equal(bits(x[0]), bits(x0[0])) and bits(tot)[0] == bits(np.float32(0.1) + np.float32(0.2))
        assert trace[0][2][0] and trace[1][2][0]
    # FILL: face 1 was never observed and takes the row of face 2, its one informed neighbour, as it is; face 2 is observed
    x, _ = ref.propagate(off, nbr, x0, 1, ref.FILL, observed_threshold=0.9)
    assert x.tolist() == [[np.float32(0.1), np.float32(0.2)], [0.5, 0.5], [0.5, 0.5]]


def test_normal_weights_by_hand():
    v = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 2, 0]], np.float32)
    n, l = ref.normals(v, [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5]])
    assert n.tolist() == [[0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 0]] and l.tolist() == [1, 1, 1, 0]
    for power in (1, 4, 16):
        def w(faces, two_sided):
            off, nbr = ref.adjacency(np.asarray(faces), 6)
            assert nbr.tolist() == [1, 0]
            return ref.normal_weights(off, nbr, v, faces, power, two_sided).tolist()
        assert w([[0, 1, 2], [0, 1, 3]], True) == [0, 0] and w([[0, 1, 2], [0, 1, 3]], False) == [0, 0]      # a right angle
        assert w([[0, 1, 2], [0, 1, 4]], True) == [1, 1] and w([[0, 1, 2], [0, 1, 4]], False) == [0, 0]      # coplanar, opposite winding
        assert w([[0, 1, 2], [1, 0, 4]], False) == [1, 1]                                                    # coplanar, same winding
        assert w([[0, 1, 2], [0, 1, 5]], True) == [0, 0]                                                     # a face without area
    # 45 degrees: q = 1 / sqrt(2) in float32 operations, then q * q * q
    v45 = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 1]], np.float32)
    faces = [[0, 1, 2], [1, 0, 3]]
    off, nbr = ref.adjacency(np.asarray(faces), 4)
    q = np.float32(1.0) / (np.float32(1.0) * np.sqrt(np.float32(2.0)))
    assert bits(ref.normal_weights(off, nbr, v45, faces, 3, False)).tolist() == bits(np.array([q * q * q] * 2)).tolist()


# ---- argument checks that need no device ---------------------------------------------------------------------------------------
def test_face_graph_refuses_wrong_arguments_before_it_needs_a_device():
    from semantic_meshes_amd import fusion
    for faces, V in ((np.zeros((4, 2), np.int32), 5), (np.zeros((4, 3), np.float32), 5), (np.full((4, 3), 5, np.int32), 5),
                     (np.full((4, 3), -1, np.int32), 5), (np.zeros((0, 3), np.int32), -1), (np.zeros(12, np.int32), 5)):
        with pytest.raises(ValueError):
            fusion.FaceGraph(faces, V)
    with pytest.raises(ValueError):
        fusion.FaceGraph.from_renderer(object(), 5)
    g = object.__new__(fusion.FaceGraph)                              # a graph that was never built: the checks come first
    g.num_faces, g.num_vertices, g.num_entries, g.device, g._h = 4, 6, 6, 0, None
    rows = np.zeros((4, 3), np.float32)
    for bad in (-1, 1.5, "3", None, True, 2 ** 32):
        with pytest.raises(ValueError):
            g.smooth(rows, iterations=bad)
        with pytest.raises(ValueError):
            g.fill_labels_device(rows, iterations=bad)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            g.smooth_sums(rows, alpha=bad)
    for bad in (np.zeros(6, np.float64), np.zeros(5, np.float32), np.zeros(7, np.float32), np.zeros((6, 1), np.float32), np.zeros(6, np.int32)):
        with pytest.raises(ValueError):
            g.smooth_labels(rows, weights=bad)
        with pytest.raises(ValueError):
            g.fill(rows, weights=bad)
    for bad in (np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32), np.zeros((4, 0), np.float32)):
        with pytest.raises(ValueError):
            g.smooth(bad)
    vertices = np.zeros((6, 3), np.float32)
    for bad in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError):
            g.normal_weights(vertices, power=bad)
        with pytest.raises(ValueError):
            g.normal_weights_host(vertices, power=bad)
    for bad in (np.zeros((5, 3), np.float32), np.zeros((6, 2), np.float32), np.zeros((6, 3), np.float64)):
        with pytest.raises(ValueError):
            g.normal_weights_host(bad)
