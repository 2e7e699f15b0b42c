"""The closest face of arbitrary points (include/smesh_points.h, fusion.SurfaceIndex / PointTransfer, data.read_ply_vertex_property),
the part that needs no GPU: the extension header and its ctypes table, the numpy reference of the GPU tests (tests/points_ref.py)
against itself in float64 and against answers derived by hand, and the PLY property reader."""
import os
import re
import subprocess

import numpy as np
import pytest

import points_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PT_HEADER = os.path.join(INCLUDE, "smesh_points.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", PT_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(PT_HEADER)
    assert declared == sorted(["smesh_surface_index_create", "smesh_surface_index_destroy", "smesh_surface_index_stats",
                               "smesh_surface_index_nearest", "smesh_point_gather", "smesh_aggregator_point_annotations"])
    assert declared == sorted(_lib.POINTS_SIGNATURES)              # every declared symbol has its ctypes signature
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    for other in sorted(os.listdir(INCLUDE)):
        if other != "smesh_points.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    assert not re.search(r"#\s*define\s+SMESH_PROF_", open(PT_HEADER).read())      # all eight slots are taken


# ---- the reference against itself ----------------------------------------------------------------------------------------------
def test_reference_in_float32_agrees_with_float64():
    """The bound guards the REFERENCE: 2^-19 is the next power of two above three times the largest |dist2_32 - dist2_64| measured
    on the CPU for 1500 triangles and 3000 points of this soup (5.1e-7; 5.5e-7 for triangles of extent 0.02)."""
    vertices, faces, points = points_ref.soup(seed=1, F=512, N=1024)
    f32, d32 = points_ref.nearest(vertices, faces, points)
    f64, d64 = points_ref.nearest(vertices, faces, points, dtype=np.float64)
    assert f32.dtype == np.int32 and d32.dtype == np.float32 and d64.dtype == np.float64
    assert (f32 >= 0).all() and np.array_equal(f32, f64)
    worst = 0.0
    for lo in range(0, len(points), 256):
        a = points_ref.dist2_all(vertices, faces, points[lo:lo + 256])
        b = points_ref.dist2_all(vertices, faces, points[lo:lo + 256], np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    print("largest |dist2_32 - dist2_64| over %d pairs: %.3g (bound %.3g)" % (len(points) * len(faces), worst, 2.0 ** -19))
    assert worst <= 2.0 ** -19


# ---- answers derived by hand ---------------------------------------------------------------------------------------------------
# the right triangle a = (0,0,0), b = (4,0,0), c = (0,4,0); every number below is exact in float32
TRI_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
REGIONS = [
    # (query point, closest point, dist2): one per case of the rule
    ((-1, -2, 0), (0, 0, 0), 5.0),         # 1: vertex a
    ((6, -1, 0), (4, 0, 0), 5.0),          # 2: vertex b
    ((1, -3, 0), (1, 0, 0), 9.0),          # 3: edge ab, t = 1/4
    ((-1, 7, 0), (0, 4, 0), 10.0),         # 4: vertex c
    ((-2, 3, 0), (0, 3, 0), 4.0),          # 5: edge ac, t = 3/4
    ((4, 4, 0), (2, 2, 0), 8.0),           # 6: edge bc, t = 1/2
    ((1, 1, 3), (1, 1, 0), 9.0),           # 7: the interior, from above the plane
]


def _region_of(q):
    """Which case of the rule fires for q against TRI_V, from the rule's own quantities in float64."""
    a, b, c = TRI_V.astype(np.float64)
    q = np.asarray(q, np.float64)
    ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
    d1, d2, d3, d4, d5, d6 = ab @ ap, ac @ ap, ab @ bp, ac @ bp, ab @ cp, ac @ cp
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [d1 <= 0 and d2 <= 0, d3 >= 0 and d4 <= d3, vc <= 0 and d1 >= 0 and d3 <= 0, d6 >= 0 and d5 <= d6,
             vb <= 0 and d2 >= 0 and d6 <= 0, va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0, True]
    return conds.index(True) + 1


def test_every_region_of_one_triangle():
    for k, (q, r, d2) in enumerate(REGIONS):
        assert _region_of(q) == k + 1
        assert float(np.sum((np.asarray(q, np.float64) - np.asarray(r, np.float64)) ** 2)) == d2      # (the hand's own arithmetic)
        for dtype in (np.float32, np.float64):
            f, d = points_ref.nearest(TRI_V, TRI_F, np.asarray([q], np.float32), dtype=dtype)
            assert f[0] == 0 and d.dtype == dtype and float(d[0]) == d2, (k + 1, q, d)
    f, d = points_ref.nearest(TRI_V, TRI_F, np.asarray([q for q, _, _ in REGIONS], np.float32))
    assert np.array_equal(f, np.zeros(7, np.int32)) and np.array_equal(d, np.asarray([r[2] for r in REGIONS], np.float32))


def test_a_point_on_a_shared_edge_gives_the_lower_face():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]], np.float32)
    for faces in ([[0, 1, 2], [1, 3, 2]], [[1, 3, 2], [0, 1, 2]]):
        f, d = points_ref.nearest(v, np.asarray(faces, np.int32), np.asarray([[2, 2, 0], [3, 1, 0], [1, 1, 0], [3, 3, 0]], np.float32))
        first = 0 if faces[0] == [0, 1, 2] else 1           # (the face that holds (1,1,0))
        assert np.array_equal(d, np.zeros(4, np.float32))
        assert f.tolist() == [0, 0, first, 1 - first]


def test_what_never_wins_and_max_distance():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.nan, 0, 0], [2, 0, 0], [np.inf, 1, 1]], np.float32)
    faces = np.array([[0, 0, 1], [0, 4, 1], [3, 1, 2], [5, 1, 2], [0, 1, 2]], np.int32)      # repeated, collinear, NaN, inf, proper
    pts = np.array([[1, 1, 1], [1, -3, 0], [np.nan, 0, 0], [9, 9, 9]], np.float32)
    f, d = points_ref.nearest(v, faces, pts)
    # (the collinear face answers (1,-3,0) from its edge ab like the proper one does: equal dist2, the lower face)
    assert f.tolist() == [4, 1, -1, 4] and d[0] == 1.0 and d[1] == 9.0 and np.isinf(d[2])
    f, d = points_ref.nearest(v, faces[:4], pts[:1] * 0 + np.float32([1, 1, 1]))
    assert f[0] >= 0 and np.isfinite(d[0])                      # (degenerate faces answer from a vertex or an edge, or not at all; never with NaN)
    assert points_ref.nearest(v, faces[2:3], pts)[0].tolist() == [-1, -1, -1, -1]      # a NaN vertex: every comparison fails, case 7, NaN
    # an infinite vertex is another matter: the products stay ordered, cases 1, 2 and 4 can fire and answer with a FINITE vertex
    f, d = points_ref.nearest(v, faces[3:4], pts)
    assert f.tolist()[:3] == [0, 0, -1] and np.isfinite(d[:2]).all()
    allinf = np.array([[np.inf, 0, 0], [0, -np.inf, 0], [np.inf, np.inf, 1]], np.float32)
    assert points_ref.nearest(allinf, np.array([[0, 1, 2]], np.int32), pts)[0].tolist() == [-1, -1, -1, -1]
    f, d = points_ref.nearest(v, faces, pts, max_distance=3.0)
    assert f.tolist() == [4, 1, -1, -1] and np.isinf(d[3])     # 9 <= 3 * 3 stays
    f, d = points_ref.nearest(v, faces, np.array([[1, 1, 0], [1, 1, 1e-3]], np.float32), max_distance=0.0)
    assert f.tolist() == [4, -1]
    assert points_ref.nearest(v, np.zeros((0, 3), np.int32), pts)[0].tolist() == [-1] * 4


# ---- data.read_ply_vertex_property ---------------------------------------------------------------------------------------------
def _write_labelled_ply(path, fmt, xyz, label, faces):
    header = ["ply", "format %s 1.0" % fmt, "comment ground truth", "element vertex %d" % len(xyz), "property float x", "property float y",
              "property float z", "property ushort label", "element face %d" % len(faces), "property list uchar int vertex_indices",
              "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        if fmt == "ascii":
            for p, l in zip(xyz, label):
                fh.write(("%r %r %r %d\n" % (float(p[0]), float(p[1]), float(p[2]), l)).encode("ascii"))
            for f in faces:
                fh.write(("3 %d %d %d\n" % tuple(f)).encode("ascii"))
        else:
            e = "<" if fmt == "binary_little_endian" else ">"
            rec = np.empty(len(xyz), dtype=[("p", e + "f4", (3,)), ("l", e + "u2")])
            rec["p"], rec["l"] = xyz, label
            fh.write(rec.tobytes())
            frec = np.empty(len(faces), dtype=[("n", "u1"), ("v", e + "i4", (3,))])
            frec["n"], frec["v"] = 3, faces
            fh.write(frec.tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_ply_vertex_property(tmp_path, fmt):
    from semantic_meshes_amd import data
    rng = np.random.default_rng(4)
    xyz = rng.random((37, 3)).astype(np.float32)
    label = rng.integers(0, 41, 37).astype(np.uint16)
    label[5] = 65535
    faces = rng.integers(0, 37, (20, 3)).astype(np.int32)
    path = str(tmp_path / "gt.ply")
    _write_labelled_ply(path, fmt, xyz, label, faces)
    got = data.read_ply_vertex_property(path, "label")
    assert got.dtype == np.uint16 and got.ndim == 1 and got.dtype.isnative and np.array_equal(got, label)
    y = data.read_ply_vertex_property(path, "y")
    assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), xyz[:, 1].copy().view(np.uint32))
    for absent in ("labels", "vertex_indices", "red"):
        with pytest.raises(ValueError):
            data.read_ply_vertex_property(path, absent)
    ply = data.Ply(path)                                        # the mesh reader still takes the file
    assert np.array_equal(ply.vertices.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(ply.faces, faces)


def test_point_transfer_refuses_wrong_arguments_before_it_needs_a_device():
    from semantic_meshes_amd import fusion
    v = np.zeros((5, 3), np.float32)
    for vertices, faces in ((np.zeros((5, 2), np.float32), np.zeros((4, 3), np.int32)), (np.zeros((5, 3), np.int32), np.zeros((4, 3), np.int32)),
                            (v, np.zeros((4, 2), np.int32)), (v, np.zeros((4, 3), np.float32)), (v, np.full((4, 3), 5, np.int32)),
                            (v, np.full((4, 3), -1, np.int32))):
        with pytest.raises(ValueError):
            fusion.SurfaceIndex(vertices, faces)
    with pytest.raises(ValueError):
        fusion.PointTransfer(None, np.zeros((3, 3), np.float32))
