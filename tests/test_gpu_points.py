"""The closest face of arbitrary points and the fused rows of those faces on the GPU (include/smesh_points.h, fusion.SurfaceIndex,
fusion.PointTransfer) against tests/points_ref.py -- the header's rule in numpy float32, the exhaustive scan -- and numpy on get().
The reference of every comparison is computed on the host, never by the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import points_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def assert_same(got, want):
    """Faces equal, dist2 equal in bits, for every point."""
    (gf, gd), (wf, wd) = got, want
    gf, gd = np.asarray(gf), np.asarray(gd)
    assert gf.dtype == np.int32 and gd.dtype == np.float32 and gf.shape == wf.shape and gd.shape == wd.shape
    assert np.array_equal(gf, wf), "%d of %d faces differ, first at point %d" % (int((gf != wf).sum()), gf.size, int(np.argmax(gf != wf)))
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), "%d of %d dist2 differ in bits" % (
        int((gd.view(np.uint32) != wd.view(np.uint32)).sum()), gd.size)


@functools.lru_cache(maxsize=None)
def soup_case():
    """The host test's soup and points plus 64 points at ten times the bounding box's extent (they start outside the grid), and the
    reference's answer.  Computed once; nobody writes to it."""
    vertices, faces, points = points_ref.soup(seed=1, F=512, N=1024)
    lo, hi = vertices.min(axis=0), vertices.max(axis=0)
    rng = np.random.default_rng(2)
    far = (0.5 * (lo + hi) + 10.0 * (hi - lo) * (rng.random((64, 3)) - 0.5)).astype(np.float32)
    points = np.concatenate([points, far])
    assert (np.abs(far - 0.5 * (lo + hi)) > 0.5 * (hi - lo)).any(axis=1).sum() > 56
    want = points_ref.nearest(vertices, faces, points)
    for a in (vertices, faces, points) + want:
        a.setflags(write=False)
    return vertices, faces, points, want


# ---- 1. soup, bit for bit ------------------------------------------------------------------------------------------------------
def test_soup_is_bit_equal_to_the_exhaustive_reference(sm):
    from semantic_meshes_amd.device import to_device
    vertices, faces, points, want = soup_case()
    assert (want[0] >= 0).all()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    st = index.stats()
    print("soup grid:", st)
    assert st["faces"] == 512 and min(st["dims"]) > 1 and st["entries"] >= 512 - st["large_faces"]
    assert_same(index.nearest(points), want)                                  # host points
    fd, dd = index.nearest_device(to_device(points))                          # device points, device results
    assert_same((fd.numpy(), dd.numpy()), want)


# ---- 2. the grid is only a shortcut --------------------------------------------------------------------------------------------
def test_the_exhaustive_kernel_gives_the_same_arrays(sm):
    from semantic_meshes_amd import _lib
    vertices, faces, points, want = soup_case()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    before = _lib.get_option("points_grid")
    assert before == 1
    try:
        _lib.set_option("points_grid", 0)
        assert _lib.get_option("points_grid") == 0
        assert_same(index.nearest(points), want)
    finally:
        _lib.set_option("points_grid", before)
    assert _lib.get_option("points_grid") == before


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_face(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(8, 8, extent=8.0, relief=0.0)                      # a 9 x 9-vertex plane of 128 triangles, integer coordinates
    v, f = mesh.vertices, mesh.faces
    assert v.shape == (81, 3) and f.shape == (128, 3) and np.array_equal(v, np.round(v)) and not v[:, 2].any()
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    assert len(edges) == 208
    points = np.concatenate([v, 0.5 * (v[edges[:, 0]] + v[edges[:, 1]])]).astype(np.float32)
    want = points_ref.nearest(v, f, points)
    assert not want[1].any()
    incident = [np.flatnonzero((f == k).any(axis=1)).min() for k in range(81)]         # the lowest face that names the vertex
    assert np.array_equal(want[0][:81], np.asarray(incident, np.int32))
    index = sm.fusion.SurfaceIndex(v, f)
    assert_same(index.nearest(points), want)


# ---- 4. sizes the grid dislikes ------------------------------------------------------------------------------------------------
def _small_triangles(rng, n, extent, lo=0.0, hi=1.0):
    centres = lo + (hi - lo) * rng.random((n, 1, 3))
    return (centres + extent * (rng.random((n, 3, 3)) - 0.5)).reshape(-1, 3).astype(np.float32)


def test_sizes_the_grid_dislikes(sm):
    rng = np.random.default_rng(3)
    points = (-0.2 + 1.4 * rng.random((300, 3))).astype(np.float32)
    # (a) one ground triangle spanning the whole box, plus 300 triangles of extent 0.01
    v = np.concatenate([np.array([[-1, -1, 0], [3, -1, 0], [-1, 3, 0]], np.float32), _small_triangles(rng, 300, 0.01)])
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    index = sm.fusion.SurfaceIndex(v, f)
    print("(a)", index.stats())
    assert index.stats()["large_faces"] >= 1
    assert_same(index.nearest(points), points_ref.nearest(v, f, points))
    # ... and the same with enough faces for a grid in which the ground triangle overlaps more than 4096 cells (the fixed number)
    v = np.concatenate([np.array([[-1, -1, 0], [3, -1, 0], [-1, 3, 0]], np.float32), _small_triangles(rng, 80000, 0.004)])
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    index = sm.fusion.SurfaceIndex(v, f)
    st = index.stats()
    print("(a, 80 k)", st)
    assert st["large_faces"] >= 1 and st["dims"][0] * st["dims"][1] > 4096 and st["dims"][0] * st["dims"][1] * 8 < np.prod(st["dims"])
    assert_same(index.nearest(points[:64]), points_ref.nearest(v, f, points[:64], chunk=16))
    # (b) 200 triangles inside a 0.001 cube, plus one vertex at distance 100: nearly everything falls in one cell
    v = np.concatenate([_small_triangles(rng, 200, 0.0002, 0.5, 0.501), np.array([[100, 0.5, 0.5]], np.float32)])
    f = np.arange(600, dtype=np.int32).reshape(-1, 3)
    index = sm.fusion.SurfaceIndex(v, f)
    print("(b)", index.stats())
    near = np.concatenate([points, (0.5 + 0.002 * (rng.random((200, 3)) - 0.25)).astype(np.float32)])
    assert_same(index.nearest(near), points_ref.nearest(v, f, near))
    # (c) a flat mesh: z == 0 for every vertex, one axis has one cell
    v = _small_triangles(rng, 300, 0.1)
    v[:, 2] = 0.0
    f = np.arange(900, dtype=np.int32).reshape(-1, 3)
    index = sm.fusion.SurfaceIndex(v, f)
    print("(c)", index.stats())
    assert index.stats()["dims"][2] == 1 and index.stats()["dims"][0] > 1
    assert_same(index.nearest(points), points_ref.nearest(v, f, points))
    # (d) F = 1, and N = 1
    v1, f1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    index1 = sm.fusion.SurfaceIndex(v1, f1)
    assert_same(index1.nearest(points), points_ref.nearest(v1, f1, points))
    assert_same(index.nearest(points[:1]), points_ref.nearest(v, f, points[:1]))
    # (e) N = 0, and F = 0
    none = np.zeros((0, 3), np.float32)
    assert_same(index.nearest(none), points_ref.nearest(v, f, none))
    for verts in (v, none):
        empty = sm.fusion.SurfaceIndex(verts, np.zeros((0, 3), np.int32))
        want = points_ref.nearest(verts, np.zeros((0, 3), np.int32), points)
        assert (want[0] == -1).all() and np.isinf(want[1]).all()
        assert_same(empty.nearest(points), want)
        assert_same(empty.nearest(none), points_ref.nearest(verts, np.zeros((0, 3), np.int32), none))


# ---- 5. faces that must never win ----------------------------------------------------------------------------------------------
def test_degenerate_and_non_finite_faces(sm):
    vertices, faces, points, _ = soup_case()
    v, f = vertices.copy(), faces.copy()
    rng = np.random.default_rng(5)
    pick = rng.choice(512, 24, replace=False)
    for k, face in enumerate(pick[:16]):
        a, b, c = f[face]
        if k % 2:
            f[face, 1] = a                                       # a repeated vertex
        else:
            v[c] = v[a] + np.float32(2.0) * (v[b] - v[a])        # three collinear vertices
    for k, face in enumerate(pick[16:]):
        v[f[face, k % 3], (k // 3) % 3] = (np.nan, np.inf, -np.inf, np.nan)[k % 4]
    pts = np.concatenate([points, v[f[pick[:16], 0]], 0.5 * (v[f[pick[:16], 0]] + v[f[pick[:16], 1]])]).astype(np.float32)
    want = points_ref.nearest(v, f, pts)
    index = sm.fusion.SurfaceIndex(v, f)
    print("degenerate:", index.stats())
    assert index.stats()["large_faces"] >= 24
    assert_same(index.nearest(pts), want)
    # a mesh of only non-finite faces: a NaN vertex anywhere, or no finite vertex at all (an infinite vertex beside finite ones can
    # still answer from those -- tests/test_points_host.py -- and is compared with the reference above)
    bad_v = vertices[:72].copy()
    for face in range(24):
        if face % 2:
            bad_v[3 * face + face % 3, face % 3] = np.nan
        else:
            bad_v[3 * face:3 * face + 3, (face // 2) % 3] = (np.inf, -np.inf)[face % 4 // 2]
    bad_f = faces[:24]
    want = points_ref.nearest(bad_v, bad_f, points)
    assert (want[0] == -1).all() and np.isinf(want[1]).all()
    assert_same(sm.fusion.SurfaceIndex(bad_v, bad_f).nearest(points), want)
    # a point with a NaN coordinate
    odd = points[:8].copy()
    odd[1, 0], odd[4, 2], odd[6, 1] = np.nan, np.inf, -np.inf
    got = sm.fusion.SurfaceIndex(vertices, faces).nearest(odd)
    assert got[0][[1, 4, 6]].tolist() == [-1, -1, -1] and np.isinf(got[1][[1, 4, 6]]).all()
    assert_same(got, points_ref.nearest(vertices, faces, odd))


# ---- 6. max_distance -----------------------------------------------------------------------------------------------------------
def test_max_distance(sm):
    vertices, faces, points, want = soup_case()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    R = np.float32(0.05)
    keep = want[1] <= R * R
    assert 50 < keep.sum() < len(points) - 50
    masked = (np.where(keep, want[0], -1).astype(np.int32), np.where(keep, want[1], np.float32(np.inf)).astype(np.float32))
    assert_same(index.nearest(points, max_distance=0.05), masked)
    assert_same(index.nearest(points, max_distance=0.05), points_ref.nearest(vertices, faces, points, max_distance=0.05))
    on = np.concatenate([points[:100], vertices[::7]])           # R = 0 keeps exactly the points with dist2 == 0
    ref = points_ref.nearest(vertices, faces, on)
    zero = ref[1] == 0
    assert zero.sum() >= len(vertices[::7]) and not zero[:100].any()
    got = index.nearest(on, max_distance=0.0)
    assert np.array_equal(got[0] >= 0, zero)
    assert_same(got, (np.where(zero, ref[0], -1).astype(np.int32), np.where(zero, ref[1], np.float32(np.inf)).astype(np.float32)))
    for bad in (-1.0, -0.0001, float("nan")):
        with pytest.raises(ValueError):
            index.nearest(points, max_distance=bad)
    with pytest.raises(ValueError):
        sm.fusion.PointTransfer(index, points, max_distance=-2.0)


# ---- 7. gather -----------------------------------------------------------------------------------------------------------------
def np_gather(rows, faces, threshold):
    """(sums float32, float64 quotients, don't-care mask, labels) of rows[faces] by the header's rule."""
    has = faces >= 0
    sums = np.where(has[:, None], rows[np.maximum(faces, 0)], np.float32(0)).astype(np.float32)
    total = np.zeros(len(faces), np.float32)
    for c in range(rows.shape[1]):                               # float32, ascending c, from 0
        total = total + sums[:, c]
    dc = ~has | (total < np.float32(threshold))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sums.astype(np.float64) / total.astype(np.float64)[:, None]
    q[dc] = 0.0
    labels = np.argmax(sums, axis=1).astype(np.int32)
    labels[dc] = -1
    return sums, q, dc, labels


def gather_rows(rng, F, C):
    rows = (rng.random((F, C), dtype=np.float32) ** 3 + np.float32(1e-3)).astype(np.float32)
    rows /= rows.sum(axis=1, keepdims=True)
    kind = rng.random(F)
    rows[kind < 0.2] = 0.0                                       # all-zero rows
    rows[(kind >= 0.2) & (kind < 0.4)] *= np.float32(0.5)        # rows below the threshold
    return rows


@pytest.mark.parametrize("C", [1, 19, 40, 150])
def test_gather(sm, C):
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.device import to_device
    vertices, faces, points, want = soup_case()
    rng = np.random.default_rng(700 + C)
    F = len(faces)
    rows = gather_rows(rng, F, C)
    pt = sm.fusion.PointTransfer(sm.fusion.SurfaceIndex(vertices, faces), points, max_distance=0.05)
    near = pt.faces.numpy()
    assert pt.num_points == len(points) and (near == -1).sum() > 50 and (near >= 0).sum() > 50
    assert_same((near, pt.dist2.numpy()), points_ref.nearest(vertices, faces, points, max_distance=0.05))
    sums, q, dc, labels = np_gather(rows, near, 0.9)
    assert dc[near >= 0].any() and (~dc).any()
    assert np.abs(rows.astype(np.float64).sum(axis=1) - 0.9).min() > 0.05          # (the inputs keep the don't-care decision honest)
    for source in (rows, to_device(rows)):
        got = pt.sums(source)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), sums.view(np.uint32))
        ann = pt.annotations(source)
        assert ann.dtype == np.float32 and np.array_equal(~ann.any(axis=1), dc)
        err = np.abs(ann.astype(np.float64) - q)
        print("annotations C=%d: max err / bound = %.3f" % (C, float((err[q > 0] / ((C + 2) * EPS * q[q > 0])).max())))
        assert (err <= (C + 2) * EPS * np.abs(q)).all()
        assert np.array_equal(pt.labels(source), labels)
        assert np.array_equal(pt.sums_device(source).numpy().view(np.uint32), sums.view(np.uint32))      # the device forms
        assert np.array_equal(pt.annotations_device(source).numpy().view(np.uint32), ann.view(np.uint32))
        assert np.array_equal(pt.labels_device(source).numpy(), labels)
    # a face index >= F, at the library
    bad = near.copy()
    bad[3] = F
    out = np.empty(len(bad), np.int32)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().smesh_point_gather(rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, F, C, bad.ctypes.data_as(ctypes.c_void_p),
                                                 len(bad), _lib.MEM_HOST, _lib.VTX_ANNOTATIONS, 0.9, None, out.ctypes.data_as(ctypes.c_void_p),
                                                 _lib.MEM_HOST))
    _lib.check(_lib.lib().smesh_point_gather(rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, F, C, near.ctypes.data_as(ctypes.c_void_p),
                                             len(near), _lib.MEM_HOST, _lib.VTX_ANNOTATIONS, 0.9, None, out.ctypes.data_as(ctypes.c_void_p),
                                             _lib.MEM_HOST))
    assert np.array_equal(out, labels)                           # host faces, through the C ABI
    for wrong in (np.zeros((F + 1, C), np.float32), np.zeros((F, C), np.float64), np.zeros(F * C, np.float32)):
        with pytest.raises(ValueError):
            pt.sums(wrong)


# ---- 8. from an aggregator -----------------------------------------------------------------------------------------------------
def _fuse(sm, agg, renderer, cams, C):
    from semantic_meshes_amd import synth
    for k, cam in enumerate(cams):
        agg.add(renderer.render(cam)[0], synth.device_probs(cam.width, cam.height, C, synth.probs_seed(11, k), 0.1))


def _np_labels(rows, faces, threshold=0.9):
    return np_gather(rows, faces, threshold)[3]


@pytest.mark.parametrize("kind", ["sum", "summax", "mul"])
def test_from_an_aggregator(sm, kind):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    F, C = len(mesh.faces), 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    agg = sm.fusion.MeshAggregator(F, C, kind)
    _fuse(sm, agg, sm.render.triangles(mesh), cams, C)
    rng = np.random.default_rng(8)
    pick = rng.integers(0, F, 500)
    w = rng.dirichlet(np.ones(3), 500)[:, :, None]
    points = ((mesh.vertices[mesh.faces[pick]] * w).sum(axis=1) + rng.normal(0, 0.05, (500, 3))).astype(np.float32)
    index = sm.fusion.SurfaceIndex.from_mesh(mesh)
    pt = sm.fusion.PointTransfer(index, points)
    faces = pt.faces.numpy()
    assert_same((faces, pt.dist2.numpy()), points_ref.nearest(mesh.vertices, mesh.faces, points))
    rows = agg.get()
    assert rows.any(axis=1).mean() > 0.3
    got = pt.sums(agg)
    assert np.array_equal(got.view(np.uint32), rows[faces].view(np.uint32))
    assert np.array_equal(pt.labels(agg), _np_labels(rows, faces))
    assert np.array_equal(pt.labels_device(agg).numpy(), _np_labels(rows, faces))
    with pytest.raises(ValueError):
        pt.labels(sm.fusion.MeshAggregator(F + 1, C, kind))                      # wrong F
    other = sm.fusion.MeshAggregator(F, C, kind)
    other.device = 1                                                             # (an aggregator that says it lives elsewhere)
    with pytest.raises(ValueError):
        pt.labels(other)
    other.device = 0


def test_from_a_texel_renderer(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    C = 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    r = sm.render.texels(mesh, cams, 2.0)
    agg = sm.fusion.MeshAggregator(r.getPrimitivesNum(), C)
    _fuse(sm, agg, r, cams, C)
    lfaces = r.texel_layout()[0]
    index = sm.fusion.SurfaceIndex.from_renderer(r, mesh.vertices)
    assert index.num_faces == len(lfaces)
    rng = np.random.default_rng(9)
    points = (mesh.vertices[rng.integers(0, len(mesh.vertices), 400)] + rng.normal(0, 0.03, (400, 3))).astype(np.float32)
    pt = sm.fusion.PointTransfer(index, points)
    faces = pt.faces.numpy()
    assert_same((faces, pt.dist2.numpy()), points_ref.nearest(mesh.vertices, lfaces, points))
    face_rows = r.face_annotations(agg)                                          # [F,C] in the layout's face order
    assert np.array_equal(pt.sums(face_rows).view(np.uint32), face_rows[faces].view(np.uint32))
    assert np.array_equal(pt.labels(r.face_annotations_device(agg)), _np_labels(face_rows, faces))
    with pytest.raises(ValueError):
        sm.fusion.SurfaceIndex.from_renderer(sm.render.triangles(mesh), mesh.vertices)
    with pytest.raises(ValueError):
        pt.labels(agg)                                                           # texels, not faces: wrong F


# ---- 9. the use it is for ------------------------------------------------------------------------------------------------------
def test_vertex_metrics_on_a_decimated_mesh(sm):
    from semantic_meshes_amd import synth
    full = synth.grid_mesh(40, 20)
    C = 19
    kept = full.faces[::2]                                                       # every second face dropped
    mesh = sm.data.Mesh(full.vertices, kept)
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    agg = sm.fusion.MeshAggregator(len(kept), C)
    _fuse(sm, agg, sm.render.triangles(mesh), cams, C)
    gt = np.random.default_rng(10).integers(-1, C, len(full.vertices)).astype(np.int32)
    pt = sm.fusion.PointTransfer(sm.fusion.SurfaceIndex.from_mesh(mesh), full.vertices)        # the ORIGINAL vertices
    cm = sm.fusion.ConfusionMatrix(C)
    cm.add(pt.labels_device(agg), gt)
    ref_faces = points_ref.nearest(mesh.vertices, kept, full.vertices)[0]
    pred = _np_labels(agg.get(), ref_faces)
    assert (pred >= 0).mean() > 0.3 and (pred == -1).any()
    want = np.zeros((C, C + 1), np.uint64)
    ok = (gt >= 0) & (gt < C)
    np.add.at(want, (gt[ok], np.where(pred[ok] >= 0, pred[ok], C)), 1)
    got = cm.get()
    assert got.shape == want.shape and np.array_equal(got, want)
