"""Per-vertex results on the GPU (include/smesh_vertices.h, fusion.VertexTransfer, PlyRendererTexels.face_annotations) against a plain
numpy restatement of eval-scannet/eval_scannet.py:249-287.  The reference of every comparison is numpy on the oracle's get() or on a
random [F, C] array, never the output of the code under test."""
import ctypes

import numpy as np
import pytest

from helpers import assert_fused_close

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def corner_mask(faces):
    """[F,3] bool: False where a corner repeats an earlier corner of its face (the reference's set per vertex, :255-258)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.ones(f.shape, bool)
    keep[:, 1] = f[:, 1] != f[:, 0]
    keep[:, 2] = (f[:, 2] != f[:, 0]) & (f[:, 2] != f[:, 1])
    return keep


def np_csr(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = corner_mask(f).ravel()
    vert = f.ravel()[keep]
    face = np.repeat(np.arange(len(f), dtype=np.uint32), 3)[keep]
    order = np.argsort(vert, kind="stable")                 # stable: the faces of a vertex stay in ascending order
    offsets = np.zeros(V + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(vert, minlength=V))
    return offsets, face[order]


def np_sums(faces, V, rows):
    """float32 [V,C]: np.add.at adds in index order, i.e. per vertex in ascending face order, one float32 addition after another."""
    rows = np.asarray(rows, np.float32)
    acc = np.zeros((V, rows.shape[1]), np.float32)
    keep = corner_mask(faces).ravel()
    np.add.at(acc, np.asarray(faces, np.int64).ravel()[keep], np.repeat(rows, 3, 0)[keep])
    return acc


def np_annotations(sums, threshold):
    """(float64 quotient of the float32 sums, don't-care mask): all-zero rows where the total is below the threshold."""
    s = sums.astype(np.float64)
    t = s.sum(axis=1)
    dc = t < threshold
    with np.errstate(invalid="ignore", divide="ignore"):
        q = s / t[:, None]
    q[dc] = 0.0
    return q, dc


def np_labels(sums, threshold):
    lab = np.argmax(sums, axis=1).astype(np.int32)
    lab[np_annotations(sums, threshold)[1]] = -1
    return lab


def assert_annotations(got, sums, threshold, C):
    """Relative error at most (C + 2) 2^-24 -- C - 1 sequential float32 additions of non-negative terms for the total and one
    correctly rounded division -- and the don't-care set exactly, no row excluded."""
    want, dc = np_annotations(sums, threshold)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(~got.any(axis=1) & dc, dc), "a don't-care row is not all zero"
    assert np.array_equal(got[~dc].sum(axis=1) > 0.5, np.ones(int((~dc).sum()), bool)), "an annotated row came out as don't care"
    err = np.abs(got.astype(np.float64) - want)
    bound = (C + 2) * EPS * np.abs(want)
    print("annotations C=%d thr=%g: max err / bound = %.3f, don't care %d of %d" % (
        C, threshold, float((err / np.maximum(bound, 1e-300))[want > 0].max()) if (want > 0).any() else 0.0, int(dc.sum()), len(dc)))
    assert (err <= bound).all()


def assert_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d of %d elements differ" % (
        int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def random_soup(rng, F=30000, V=9000, hub_valence=10000):
    """Faces with a repeated vertex, vertices without faces (the last 500 are never named) and one hub vertex shared by
    `hub_valence` faces."""
    faces = rng.integers(0, V - 500, size=(F, 3)).astype(np.int32)
    faces[faces == 7] = 8                                     # vertex 7 is the hub: exactly the faces below
    twice = rng.choice(F, 600, replace=False)
    faces[twice, 1] = faces[twice, 0]
    thrice = rng.choice(F, 40, replace=False)
    faces[thrice] = faces[thrice, :1]
    hub = rng.choice(F, hub_valence, replace=False)
    faces[hub, rng.integers(0, 3, hub_valence)] = 7
    assert (~corner_mask(faces)).sum() > 100
    return faces, V


def normalised_rows(rng, n, C, zero_fraction=0.3):
    """L1-normalised float32 rows, `zero_fraction` of them all zero: a vertex total is a whole number of annotated faces to within
    rounding, never near the thresholds 0.9 and 1.5."""
    raw = (rng.random((n, C), dtype=np.float32) ** 3 + np.float32(1e-3)).astype(np.float32)
    raw[rng.random(n) < zero_fraction] = 0.0
    return raw


def oracle_rows(oracle, kind, raw):
    """The oracle's get() after set_raw of the raw state."""
    o = oracle.OracleAggregator(raw.shape[0], raw.shape[1], kind)
    o.set_raw(raw)
    return o.get()


CLASS_COUNTS = [1, 3, 6, 12, 19, 40, 64, 65, 150, 256, 300, 600]      # (600: beyond the rows whose sums stay in registers)
# the wave-wide instances that hold 6, 7 and 8 chunks of 64 classes per lane (k_vertex_gather<64, 6 .. 8>: 321 .. 512 classes), and
# the last count that stays in registers
WIDE_CLASS_COUNTS = [321, 385, 449, 512]


# ---- 1. adjacency ---------------------------------------------------------------------------------------------------------------
def test_adjacency_equals_the_numpy_csr(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(60, 30)
    soup, V = random_soup(np.random.default_rng(1))
    cases = [(mesh.faces, len(mesh.vertices)), (soup, V), (np.zeros((0, 3), np.int32), 0), (np.zeros((0, 3), np.int32), 17)]
    for faces, nv in cases:
        vt = sm.fusion.VertexTransfer(faces, nv)
        offsets, adj = vt.adjacency()
        want_off, want_adj = np_csr(faces, nv)
        assert offsets.dtype == np.uint64 and adj.dtype == np.uint32
        assert np.array_equal(offsets, want_off)
        assert np.array_equal(adj, want_adj)
    offsets, _ = sm.fusion.VertexTransfer(soup, V).adjacency()
    assert int(offsets[8] - offsets[7]) == 10000 and (np.diff(offsets.astype(np.int64))[-500:] == 0).all()
    vt = sm.fusion.VertexTransfer.from_mesh(mesh)
    assert np.array_equal(vt.adjacency()[1], np_csr(mesh.faces, len(mesh.vertices))[1])


# ---- 2. sums, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASS_COUNTS + WIDE_CLASS_COUNTS)
def test_sums_are_bit_equal(sm, oracle, C):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(100 + C)
    faces, V = random_soup(rng, F=12000, V=4000, hub_valence=3000)
    F = len(faces)
    vt = sm.fusion.VertexTransfer(faces, V)
    raw = normalised_rows(rng, F, C)
    rows = oracle_rows(oracle, "sum", raw)
    assert ((rows.sum(axis=1) == 0).mean() > 0.2) and np.abs(rows.sum(axis=1)[rows.any(axis=1)] - 1).max() < 1e-5
    want = np_sums(faces, V, rows)
    assert_bits(vt.sums(rows), want)                           # host array
    assert_bits(vt.sums(to_device(rows)), want)                # device array
    plain = rng.random((F, C), dtype=np.float32)               # (not normalised: any float32 rows)
    assert_bits(vt.sums(plain), np_sums(faces, V, plain))
    for kind in ("sum", "summax"):
        agg = sm.fusion.MeshAggregator(F, C, kind)
        agg.set_raw(raw)
        assert_bits(vt.sums(agg), np_sums(faces, V, oracle_rows(oracle, kind, raw)))


# ---- 3. annotations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_annotations_within_the_derived_bound(sm, oracle, C):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(200 + C)
    faces, V = random_soup(rng, F=12000, V=4000, hub_valence=3000)
    F = len(faces)
    vt = sm.fusion.VertexTransfer(faces, V)
    raw = normalised_rows(rng, F, C)
    rows = oracle_rows(oracle, "sum", raw)
    sums = np_sums(faces, V, rows)
    assert_bits(vt.sums(rows), sums)
    totals = sums.astype(np.float64).sum(axis=1)
    for thr in (0.9, 1.5):
        assert np.abs(totals - thr).min() > 0.09               # (the inputs keep the don't-care decision honest)
        assert_annotations(vt.annotations(rows, thr), sums, thr, C)
        assert_annotations(vt.annotations_device(to_device(rows), thr).numpy(), sums, thr, C)
    agg = sm.fusion.MeshAggregator(F, C, "summax")
    agg.set_raw(raw)
    assert_annotations(vt.annotations(agg), np_sums(faces, V, oracle_rows(oracle, "summax", raw)), 0.9, C)


def test_annotations_from_a_mul_aggregator(sm, oracle):
    rng = np.random.default_rng(7)
    faces, V = random_soup(rng, F=12000, V=4000, hub_valence=3000)
    F, C = len(faces), 19
    raw = (-4.0 * rng.random((F, C), dtype=np.float32)).astype(np.float32)     # log-probabilities
    agg = sm.fusion.MeshAggregator(F, C, "mul")
    agg.set_raw(raw)
    vt = sm.fusion.VertexTransfer(faces, V)
    want, dc = np_annotations(np_sums(faces, V, oracle_rows(oracle, "mul", raw)), 0.9)
    got = vt.annotations(agg)
    assert np.array_equal(~got.any(axis=1), dc)
    assert_fused_close(got, want)


# ---- 4. labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 6, 12, 19, 64, 150, 300, 600])
def test_labels_are_the_argmax_of_the_sums_with_ties(sm, C):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(300 + C)
    faces, V = random_soup(rng, F=12000, V=4000, hub_valence=3000)
    F = len(faces)
    # dyadic rows: two classes at 1/2 or four at 1/4 (or all zero) -- every sum is exact, so equal sums are exactly equal
    rows = np.zeros((F, C), np.float32)
    for f in range(F):
        u = rng.random()
        if u < 0.3:
            continue
        k = 2 if (u < 0.65 or C < 4) else 4
        rows[f, rng.choice(min(C, 6), k, replace=False)] = 1.0 / k
    vt = sm.fusion.VertexTransfer(faces, V)
    sums = np_sums(faces, V, rows)
    assert_bits(vt.sums(rows), sums)
    top = sums.max(axis=1)
    assert ((sums == top[:, None]).sum(axis=1)[top > 0] > 1).sum() > 100          # rows with exact ties
    for thr in (0.9, 1.5):
        want = np_labels(sums, thr)
        assert (want == -1).any() and (want >= 0).any()
        got = vt.labels(rows, thr)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert np.array_equal(vt.labels_device(to_device(rows), thr).numpy(), want)
    agg = sm.fusion.MeshAggregator(F, C, "sum")
    agg.set_raw(rows)
    assert np.array_equal(vt.labels(agg), np_labels(sums, 0.9))


def test_labels_only_allocates_no_vertex_rows(sm):
    """1 M faces, C = 19: a labels-only call must not raise the device's allocated bytes by V * C * 4.  Every block a call allocates
    and gives back sits in the library's allocator cache afterwards, and device.trim() reports (and empties) that cache."""
    from semantic_meshes_amd import device, synth
    mesh = synth.grid_mesh(1000, 500)
    F, V, C = len(mesh.faces), len(mesh.vertices), 19
    vt = sm.fusion.VertexTransfer.from_mesh(mesh)
    rows = device.to_device(normalised_rows(np.random.default_rng(5), F, C))
    agg = sm.fusion.MeshAggregator(F, C)
    agg.set_raw(rows.numpy())
    for source in (rows, agg):
        device.trim()
        lab = vt.labels_device(source)
        assert lab.shape == (V,)
        del lab
        host = vt.labels(source)
        held = device.trim()
        print("labels only: %d bytes went through the allocator, V*C*4 = %d" % (held, V * C * 4))
        assert held < V * C * 4
        assert (host >= -1).all() and (host < C).all()
    device.trim()
    ann = vt.annotations_device(rows)
    del ann
    assert device.trim() >= V * C * 4                           # (the measurement sees a [V,C] buffer when there is one)


def test_a_vertex_without_faces_is_dont_care_whatever_the_threshold(sm):
    rng = np.random.default_rng(9)
    faces, V = random_soup(rng, F=12000, V=4000, hub_valence=3000)
    bare = np.diff(np_csr(faces, V)[0].astype(np.int64)) == 0
    assert bare.sum() >= 500
    rows = rng.random((len(faces), 19), dtype=np.float32) + np.float32(0.01)        # (every face annotated: every total positive)
    vt = sm.fusion.VertexTransfer(faces, V)
    for thr in (0.0, -1.0):
        lab, ann = vt.labels(rows, thr), vt.annotations(rows, thr)
        assert np.array_equal(lab == -1, bare) and np.array_equal(lab[~bare], np.argmax(np_sums(faces, V, rows), axis=1)[~bare])
        assert np.isfinite(ann).all() and not ann[bare].any() and (ann[~bare].sum(axis=1) > 0.99).all()


# ---- 5. texels ------------------------------------------------------------------------------------------------------------------
def test_texel_face_annotations_and_vertex_transfer_from_the_renderer(sm, oracle):
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.device import to_device
    W, H, C = 1296, 968, 40
    mesh = synth.grid_mesh(400, 300)
    cams = [synth.ring_camera(k, 7, W, H) for k in (0, 2, 5)]
    r = sm.render.texels(mesh, cams, 0.6)
    lfaces, res, first = r.texel_layout()
    P, F, V = r.getPrimitivesNum(), len(lfaces), len(mesh.vertices)
    n = res.astype(np.int64) * (res.astype(np.int64) + 1) // 2
    assert np.array_equal(first.astype(np.int64), np.cumsum(n) - n) and int(n.sum()) == P and res.max() > 1
    rng = np.random.default_rng(11)
    texel_raw = normalised_rows(rng, P, C)
    texel_rows = oracle_rows(oracle, "sum", texel_raw)
    want = np.zeros((F, C), np.float32)
    np.add.at(want, np.repeat(np.arange(F), n), texel_rows)    # ascending texel order, one float32 addition after another
    assert_bits(r.face_annotations(texel_rows, normalize=False), want)
    assert_bits(r.face_annotations_device(to_device(texel_rows), normalize=False).numpy(), want)
    for thr in (0.9, 1.5):
        assert np.abs(want.astype(np.float64).sum(axis=1) - thr).min() > 0.09
        assert_annotations(r.face_annotations(texel_rows, thr), want, thr, C)
    agg = sm.fusion.MeshAggregator(P, C)
    agg.set_raw(texel_raw)
    assert_annotations(r.face_annotations(agg), want, 0.9, C)

    # end to end: texels -> faces -> vertices, everything after the texel rows on the device
    vt = sm.fusion.VertexTransfer.from_renderer(r, V)
    assert np.array_equal(vt.adjacency()[1], np_csr(lfaces, V)[1])
    face_dev = r.face_annotations_device(to_device(texel_rows))
    ref_face, _ = np_annotations(want, 0.9)
    ref_sums = np_sums(lfaces, V, ref_face.astype(np.float32))
    ref_ann, ref_dc = np_annotations(ref_sums, 0.9)
    got = vt.annotations(face_dev)
    assert np.array_equal(~got.any(axis=1), ref_dc)
    assert_fused_close(got, ref_ann)
    labels = vt.labels(face_dev)
    part = np.partition(ref_sums, C - 2, axis=1)
    clear = (part[:, C - 1] - part[:, C - 2]) > 1e-4            # (the face rows are equal to rounding only: leave near-ties out)
    assert np.array_equal(labels == -1, ref_dc)
    assert np.array_equal(labels[clear & ~ref_dc], np.argmax(ref_sums, axis=1)[clear & ~ref_dc]) and clear.mean() > 0.9


# ---- 6. size --------------------------------------------------------------------------------------------------------------------
def test_one_million_faces(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(1000, 500)
    F, V, C = len(mesh.faces), len(mesh.vertices), 19
    assert (F, V) == (1000000, 501501)
    vt = sm.fusion.VertexTransfer.from_mesh(mesh)
    offsets, adj = vt.adjacency()
    valence = np.diff(offsets.astype(np.int64)).reshape(1001, 501)
    assert (valence[1:-1, 1:-1] == 6).all() and len(adj) == 3 * F
    rows = normalised_rows(np.random.default_rng(6), F, C)
    rows /= np.maximum(rows.sum(axis=1, keepdims=True), np.float32(1e-30))
    sums = np_sums(mesh.faces, V, rows)
    assert_bits(vt.sums(rows), sums)
    assert np.array_equal(vt.labels(rows), np_labels(sums, 0.9))


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_are_value_errors(sm):
    from semantic_meshes_amd import _lib, synth
    mesh = synth.grid_mesh(20, 10)
    F, V = len(mesh.faces), len(mesh.vertices)
    vt = sm.fusion.VertexTransfer.from_mesh(mesh)
    with pytest.raises(ValueError):
        vt.labels(sm.fusion.MeshAggregator(F + 1, 5))                            # P != F
    with pytest.raises(ValueError):
        vt.sums(np.zeros((F + 1, 5), np.float32))
    with pytest.raises(ValueError):
        vt.sums(np.zeros((F, 5), np.float64))                                    # dtype
    with pytest.raises(ValueError):
        vt.sums(np.zeros(F * 5, np.float32))                                     # rank
    with pytest.raises(ValueError):
        vt.sums(np.zeros((F, 0), np.float32))                                    # no classes
    lib = _lib.lib()
    rows, out = np.zeros((F, 5), np.float32), np.zeros((V, 5), np.float32)
    with pytest.raises(ValueError):                                              # wrong C, at the library
        _lib.check(lib.smesh_vertex_map_gather(vt._h, rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, 0, 0, 0.9,
                                               out.ctypes.data_as(ctypes.c_void_p), None, _lib.MEM_HOST))
    with pytest.raises(ValueError):                                              # no output asked for
        _lib.check(lib.smesh_vertex_map_gather(vt._h, rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, 5, 0, 0.9, None, None, _lib.MEM_HOST))
    agg = sm.fusion.MeshAggregator(F + 4, 5)
    with pytest.raises(ValueError):                                              # P != F, at the library
        _lib.check(lib.smesh_aggregator_vertex_annotations(agg._h, vt._h, 0, 0.9, out.ctypes.data_as(ctypes.c_void_p), None, _lib.MEM_HOST))
    bad = mesh.faces.copy()
    bad[3, 1] = V
    with pytest.raises(ValueError):
        sm.fusion.VertexTransfer(bad, V)
    h = ctypes.c_void_p()
    with pytest.raises(ValueError):                                              # a face index >= V, at the library
        _lib.check(lib.smesh_vertex_map_create(bad.ctypes.data_as(ctypes.c_void_p), F, V, 0, ctypes.byref(h)))
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        _lib.check(lib.smesh_vertex_map_create(bad.ctypes.data_as(ctypes.c_void_p), F, V, 0, ctypes.byref(h)))
    tri = sm.render.triangles(mesh)
    with pytest.raises(ValueError):                                              # a non-texel renderer
        sm.render.PlyRendererTexels.face_annotations(tri, np.zeros((F, 5), np.float32))
    with pytest.raises(ValueError):
        _lib.check(lib.smesh_renderer_texel_face_rows(tri._h, rows.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, 5, 0, 0.9,
                                                      out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
    with pytest.raises(ValueError):
        sm.fusion.VertexTransfer.from_renderer(tri, V)
