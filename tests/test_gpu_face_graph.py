"""Mesh-graph operations on the GPU (include/smesh_face_graph.h, fusion.FaceGraph) against tests/face_graph_ref.py, the header's
rule in numpy float32 by another route.  The reference of every comparison is computed on the host, never by the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import face_graph_ref as ref
import test_gpu_vertices as tv

pytestmark = pytest.mark.gpu

CLASS_COUNTS = [1, 5, 19, 32, 33, 40, 64, 65, 150, 513]      # every group width, the register-chunk form, chunk after chunk
ITERATIONS = [0, 1, 2, 7]
THRESHOLD = 0.9


# ---- inputs (computed once; nobody writes to them) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case():
    """A 40 x 30 grid of quads split into triangles, bent along the line x = 0 so that creases exist."""
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 30)
    v = mesh.vertices.astype(np.float32).copy()
    v[:, 2] += np.float32(0.8) * np.abs(v[:, 0])
    faces = np.ascontiguousarray(mesh.faces, np.int32)
    assert faces.shape == (2400, 3)
    return _case(faces, v)


@functools.lru_cache(maxsize=None)
def soup_case():
    """A soup in the style of test_gpu_vertices.random_soup: 30 000 faces over few enough vertices that most edges are shared, with
    repeated vertices, 500 unused vertices, one hub vertex of 3 000 faces, one edge shared by 40 faces and a few duplicate faces."""
    rng = np.random.default_rng(21)
    F, V = 30000, 800
    faces = rng.integers(0, V - 500, size=(F, 3)).astype(np.int32)
    faces[faces == 7] = 8                                     # vertex 7 is the hub: exactly the faces below
    twice = rng.choice(F, 600, replace=False)
    faces[twice, 1] = faces[twice, 0]
    thrice = rng.choice(F, 40, replace=False)
    faces[thrice] = faces[thrice, :1]
    hub = rng.choice(F, 3000, replace=False)
    faces[hub, rng.integers(0, 3, 3000)] = 7
    shared = rng.choice(np.setdiff1d(np.arange(F), hub), 40, replace=False)      # the edge {11, 12} in 40 faces
    faces[shared, 0], faces[shared, 1] = 11, 12
    dup = rng.choice(F, 12, replace=False)
    faces[dup[:6]] = faces[dup[6:]]                            # six faces listed twice
    vertices = (rng.random((V, 3), dtype=np.float32) + np.float32(0.25)).astype(np.float32)
    return _case(faces, vertices)


def _case(faces, vertices):
    V = len(vertices)
    offsets, nbr = ref.adjacency(faces, V)
    for a in (faces, vertices, offsets, nbr):
        a.setflags(write=False)
    return faces, vertices, V, offsets, nbr


def make_rows(rng, F, C):
    """Non-negative float32 rows: a third all zero, a tenth with a total of 0.3 (below the threshold), the others with total 1."""
    rows = (rng.random((F, C), dtype=np.float32) ** 3 + np.float32(1e-3)).astype(np.float32)
    rows /= rows.sum(axis=1, keepdims=True)
    kind = rng.random(F)
    rows[kind < 1 / 3] = 0.0
    rows[kind > 0.9] *= np.float32(0.3)
    return rows


def make_weights(rng, offsets, nbr):
    """float32 weights in [0, 2): zero on a tenth of the entries and on every entry of a twentieth of the faces."""
    w = (2.0 * rng.random(len(nbr))).astype(np.float32)
    w[rng.random(len(nbr)) < 0.1] = 0.0
    off = offsets.astype(np.int64)
    for f in np.flatnonzero(rng.random(len(off) - 1) < 0.05):
        w[off[f]:off[f + 1]] = 0.0
    return w


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "%d of %d elements differ" % (int((bits(got) != bits(want)).sum()), got.size)


# (mode, alpha, weighted) for every T of ITERATIONS
CONFIGS = [(ref.SMOOTH, 0.5, False), (ref.SMOOTH, 0.5, True), (ref.SMOOTH, 0.0, True), (ref.SMOOTH, 1.0, False),
           (ref.FILL, 0.0, False), (ref.FILL, 0.0, True)]


def check_propagation(sm, case, C, seed, configs, iterations, branch_seen):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = case
    F = len(faces)
    rng = np.random.default_rng(seed)
    rows = make_rows(rng, F, C)
    w = make_weights(rng, offsets, nbr)
    rows_before = rows.copy()
    graph = sm.fusion.FaceGraph(faces, V)
    d_rows, d_w = to_device(rows), to_device(w)
    for mode, alpha, weighted in configs:
        for T in iterations:
            trace = []
            want, tot = ref.propagate(offsets, nbr, rows, T, mode, alpha=alpha, observed_threshold=THRESHOLD, weights=w if weighted else None,
                                      trace=trace)
            labels, dc, unreached = ref.finish(want, tot, THRESHOLD)
            if mode == ref.FILL:
                weak = (ref.row_totals(rows) > 0) & (ref.row_totals(rows) < np.float32(THRESHOLD))
                for kept, averaged, stayed in trace:
                    for k, mask in enumerate((kept, averaged & ~weak, averaged & weak, stayed)):
                        branch_seen[k] = branch_seen[k] or bool(mask.any())
            for source, wts in ((rows, w), (d_rows, d_w)):
                wts = wts if weighted else None
                if mode == ref.SMOOTH:
                    sums, n1 = graph.smooth_sums(source, T, alpha, wts, return_unreached=True)
                    got_labels, n2 = graph.smooth_labels(source, T, alpha, wts, THRESHOLD, return_unreached=True)
                else:
                    sums, n1 = graph.fill_sums(source, T, THRESHOLD, wts, return_unreached=True)
                    got_labels, n2 = graph.fill_labels(source, T, THRESHOLD, wts, THRESHOLD, return_unreached=True)
                assert_bits(sums, want)
                assert got_labels.dtype == np.int32 and np.array_equal(got_labels, labels)        # the don't-care set is labels == -1
                assert (n1, n2) == (unreached, unreached)
    assert np.array_equal(bits(rows), bits(rows_before)) and np.array_equal(bits(d_rows.numpy()), bits(rows_before))
    assert np.array_equal(bits(d_w.numpy()), bits(w))
    return graph, rows, w, d_rows, d_w


# ---- 1. the graph --------------------------------------------------------------------------------------------------------------
def test_adjacency_equals_the_restatement(sm):
    from semantic_meshes_amd import _lib
    one = (np.array([[0, 1, 2]], np.int32), np.zeros((3, 3), np.float32), 3) + ref.adjacency(np.array([[0, 1, 2]]), 3)
    none = (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), 0) + ref.adjacency(np.zeros((0, 3), np.int32), 0)
    none17 = (np.zeros((0, 3), np.int32), np.zeros((17, 3), np.float32), 17) + ref.adjacency(np.zeros((0, 3), np.int32), 17)
    for faces, vertices, V, want_off, want_nbr in (grid_case(), soup_case(), one, none, none17):
        graph = sm.fusion.FaceGraph(faces, V)
        offsets, nbr = graph.adjacency()
        assert offsets.dtype == np.uint64 and nbr.dtype == np.uint32
        assert np.array_equal(offsets, want_off) and np.array_equal(nbr, want_nbr)
        F, VV, nnz = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(_lib.lib().smesh_face_graph_size(graph._h, ctypes.byref(F), ctypes.byref(VV), ctypes.byref(nnz)))
        assert (F.value, VV.value, nnz.value) == (len(faces), V, len(want_nbr)) == (graph.num_faces, graph.num_vertices, graph.num_entries)
    # what the soup is for: the scan spans several tiles of 1024, a long list, a list with repeats, the hub
    faces, _, V, off, nbr = soup_case()
    deg = np.diff(off.astype(np.int64))
    assert len(faces) > 8 * 1024 and deg.max() >= 39 and (deg == 0).any()
    assert int((faces == 7).any(axis=1).sum()) >= 2990
    assert any(len(set(nbr[int(off[f]):int(off[f + 1])].tolist())) < deg[f] for f in np.flatnonzero(deg > 1))
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 30)
    assert np.array_equal(sm.fusion.FaceGraph.from_mesh(mesh).adjacency()[1], grid_case()[4])


def test_an_index_out_of_range_is_refused(sm):
    from semantic_meshes_amd import _lib
    faces, _, V, _, _ = grid_case()
    h = ctypes.c_void_p()
    for value in (V, -1):
        bad = faces.copy()
        bad[3, 1] = value
        with pytest.raises(ValueError):
            sm.fusion.FaceGraph(bad, V)
        with pytest.raises(ValueError):                                          # at the library
            _lib.check(_lib.lib().smesh_face_graph_create(bad.ctypes.data_as(ctypes.c_void_p), len(bad), V, 0, ctypes.byref(h)))
        assert not h.value


# ---- 2. propagation, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_propagation_on_the_grid_is_bit_equal(sm, C):
    seen = [False] * 4
    check_propagation(sm, grid_case(), C, 400 + C, CONFIGS, ITERATIONS, seen)
    assert seen == [True] * 4, "a branch of FILL was never taken (kept, averaged from zero, averaged from weak, stayed): %s" % seen


@pytest.mark.parametrize("C", [19, 40])
def test_propagation_on_the_soup_is_bit_equal(sm, C):
    seen = [False] * 4
    check_propagation(sm, soup_case(), C, 500 + C, [CONFIGS[1], CONFIGS[5]] if C == 19 else [CONFIGS[0], CONFIGS[4]], ITERATIONS, seen)
    assert seen == [True] * 4, seen


def test_one_face_and_two_calls(sm):
    graph = sm.fusion.FaceGraph(np.array([[0, 1, 2]], np.int32), 3)
    x0 = np.array([[0.25, 0.0, 0.5]], np.float32)
    for T in (0, 3):
        assert_bits(graph.smooth_sums(x0, T), x0)
        assert_bits(graph.fill_sums(x0, T), x0)
    assert graph.fill_labels(x0, 2, return_unreached=True)[1] == 0 and graph.fill_labels(x0, 2).tolist() == [-1]
    assert graph.fill_labels(0 * x0, 2, return_unreached=True)[1] == 1
    faces, _, V, offsets, nbr = soup_case()
    rng = np.random.default_rng(3)
    rows, w = make_rows(rng, len(faces), 19), make_weights(rng, offsets, nbr)
    graph = sm.fusion.FaceGraph(faces, V)
    a, b = graph.smooth_sums(rows, 7, 0.5, w), graph.smooth_sums(rows, 7, 0.5, w)
    assert np.array_equal(bits(a), bits(b))
    a, b = graph.fill_sums_device(rows, 7, 0.9, w).numpy(), graph.fill_sums_device(rows, 7, 0.9, w).numpy()
    assert np.array_equal(bits(a), bits(b))


# ---- 3. annotations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_annotations_within_the_bound_of_one_division(sm, C):
    from semantic_meshes_amd.device import to_device
    faces, _, V, offsets, nbr = grid_case()
    rng = np.random.default_rng(600 + C)
    rows = make_rows(rng, len(faces), C)
    graph = sm.fusion.FaceGraph(faces, V)
    for mode, T in ((ref.SMOOTH, 2), (ref.FILL, 7), (ref.SMOOTH, 0)):
        want, tot = ref.propagate(offsets, nbr, rows, T, mode, alpha=0.5, observed_threshold=THRESHOLD)
        totals = want.astype(np.float64).sum(axis=1)
        # (the inputs keep the don't-care decision honest: a threshold that no total comes near, in float64 and in float32)
        thr = next(t for t in (0.9, 0.8, 0.7, 0.6, 0.5) if np.abs(totals - t).min() > 1e-3)
        for source in (rows, to_device(rows)):
            if mode == ref.SMOOTH:
                got, dev = graph.smooth(source, T, 0.5, None, thr), graph.smooth_device(source, T, 0.5, None, thr)
            else:
                got, dev = graph.fill(source, T, THRESHOLD, None, thr), graph.fill_device(source, T, THRESHOLD, None, thr)
            tv.assert_annotations(got, want, thr, C)
            assert np.array_equal(bits(dev.numpy()), bits(got))


# ---- 4. from an aggregator, from a texel renderer -------------------------------------------------------------------------------
def _fuse(sm, agg, renderer, cams, C):
    from semantic_meshes_amd import synth
    for k, cam in enumerate(cams):
        agg.add(renderer.render(cam)[0], synth.device_probs(cam.width, cam.height, C, synth.probs_seed(11, k), 0.1))


@pytest.mark.parametrize("kind", ["sum", "summax", "mul"])
def test_from_an_aggregator(sm, kind):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    F, C = len(mesh.faces), 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    graph = sm.fusion.FaceGraph.from_mesh(mesh)
    offsets, nbr = ref.adjacency(mesh.faces, len(mesh.vertices))
    agg = sm.fusion.MeshAggregator(F, C, kind)
    _fuse(sm, agg, sm.render.triangles(mesh), cams, C)
    pending = len(agg._pending)
    first = graph.smooth(agg, 3, 0.5)                                            # deferred views are handed over first, as get() does
    assert pending == 0 or not agg._pending
    raw = agg.get_raw().copy()
    rows = agg.get()
    assert rows.any(axis=1).mean() > 0.3
    assert np.array_equal(bits(first), bits(graph.smooth(rows, 3, 0.5)))
    want, tot = ref.propagate(offsets, nbr, rows, 3, ref.SMOOTH, alpha=0.5)
    assert_bits(graph.smooth_sums(agg, 3, 0.5), want)
    assert np.array_equal(graph.smooth_labels_device(agg, 3, 0.5).numpy(), ref.finish(want, tot, 0.9)[0])
    want, tot = ref.propagate(offsets, nbr, rows, 5, ref.FILL, observed_threshold=0.9)
    got, unreached = graph.fill_sums(agg, 5, return_unreached=True)
    assert_bits(got, want)
    assert unreached == ref.finish(want, tot, 0.9)[2]
    assert np.array_equal(bits(agg.get_raw()), bits(raw)) and np.array_equal(bits(agg.get()), bits(rows))      # the accumulator is untouched
    with pytest.raises(ValueError):
        graph.smooth(sm.fusion.MeshAggregator(F + 1, C, kind))                   # P != F
    other = sm.fusion.MeshAggregator(F, C, kind)
    other.device = 1                                                             # (an aggregator that says it lives elsewhere)
    with pytest.raises(ValueError):
        graph.smooth_labels(other)
    other.device = 0


def test_a_pending_deferred_view_is_handed_over_first(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    F, C = len(mesh.faces), 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    graph = sm.fusion.FaceGraph.from_mesh(mesh)
    agg, twin = sm.fusion.MeshAggregator(F, C), sm.fusion.MeshAggregator(F, C)
    agg.defer = True
    renderer = sm.render.triangles(mesh)
    _fuse(sm, agg, renderer, cams, C)
    _fuse(sm, twin, renderer, cams, C)
    assert len(agg._pending) == 3                                                # nothing has reached the library yet
    got = graph.smooth_sums(agg, 2, 0.5)
    assert not agg._pending
    rows = twin.get()
    assert rows.any()
    want, _ = ref.propagate(*ref.adjacency(mesh.faces, len(mesh.vertices)), rows, 2, ref.SMOOTH, alpha=0.5)
    assert_bits(got, want)


def test_from_a_texel_renderer(sm):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    C, V = 19, len(mesh.vertices)
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    r = sm.render.texels(mesh, cams, 2.0)
    agg = sm.fusion.MeshAggregator(r.getPrimitivesNum(), C)
    _fuse(sm, agg, r, cams, C)
    lfaces = r.texel_layout()[0]
    graph = sm.fusion.FaceGraph.from_renderer(r, V)
    offsets, nbr = ref.adjacency(lfaces, V)
    got_off, got_nbr = graph.adjacency()
    assert graph.num_faces == len(lfaces) and np.array_equal(got_off, offsets) and np.array_equal(got_nbr, nbr)
    face_rows = r.face_annotations(agg)                                          # [F,C] in the layout's face order
    assert face_rows.any() and (~face_rows.any(axis=1)).any()
    want, tot = ref.propagate(offsets, nbr, face_rows, 4, ref.FILL, observed_threshold=0.9)
    assert_bits(graph.fill_sums(face_rows, 4), want)
    assert np.array_equal(graph.fill_labels(r.face_annotations_device(agg), 4), ref.finish(want, tot, 0.9)[0])
    with pytest.raises(ValueError):
        sm.fusion.FaceGraph.from_renderer(sm.render.triangles(mesh), V)
    with pytest.raises(ValueError):
        graph.fill_labels(agg)                                                   # texels, not faces: wrong F


# ---- 5. normal weights ---------------------------------------------------------------------------------------------------------
def test_normal_weights_equal_the_restatement(sm):
    from semantic_meshes_amd.device import to_device
    for case in (grid_case(), soup_case()):
        faces, vertices, V, offsets, nbr = case
        n, l = ref.normals(vertices, faces)
        tiny = np.finfo(np.float32).tiny
        assert not ((np.abs(n) > 0) & (np.abs(n) < tiny)).any() and np.isfinite(n).all()      # no subnormal component
        graph = sm.fusion.FaceGraph(faces, V)
        before = vertices.copy()
        for power, two_sided in ((4, True), (1, False), (16, True), (3, False)):
            want = ref.normal_weights(offsets, nbr, vertices, faces, power, two_sided)
            dev = graph.normal_weights(vertices, power, two_sided)
            assert dev.shape == (len(nbr),) and dev.dtype == np.float32
            assert_bits(dev.numpy(), want)
            assert_bits(graph.normal_weights_host(to_device(vertices), power, two_sided), want)
        assert np.array_equal(bits(vertices), bits(before))
    faces, vertices, V, offsets, nbr = grid_case()
    w = ref.normal_weights(offsets, nbr, vertices, faces)
    assert (w < 0.9).any() and (w > 0.99).any() and (w <= 1).all() and (w >= 0).all()       # creases, and flat neighbours
    faces, vertices, V, offsets, nbr = soup_case()
    assert (ref.normal_weights(offsets, nbr, vertices, faces) == 0).any()                    # faces without area
    # the weights go straight back in
    graph = sm.fusion.FaceGraph(faces, V)
    rows = make_rows(np.random.default_rng(4), len(faces), 19)
    dw = graph.normal_weights(vertices)
    want, _ = ref.propagate(offsets, nbr, rows, 2, ref.SMOOTH, alpha=0.5, weights=ref.normal_weights(offsets, nbr, vertices, faces))
    assert_bits(graph.smooth_sums(rows, 2, 0.5, dw), want)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_are_value_errors(sm):
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = grid_case()
    F = len(faces)
    graph = sm.fusion.FaceGraph(faces, V)
    rows = np.zeros((F, 5), np.float32)
    with pytest.raises(ValueError):
        graph.smooth(rows, weights=to_device(np.zeros(len(nbr) + 1, np.float32)))
    with pytest.raises(ValueError):
        graph.smooth(rows, weights=to_device(np.zeros(len(nbr), np.int32)))
    with pytest.raises(ValueError):
        graph.smooth(np.zeros((F + 1, 5), np.float32))
    lib = _lib.lib()
    out = np.zeros((F, 5), np.float32)
    prow, pout = rows.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for C, mode, alpha, out_mode, po in ((0, 0, 0.5, 0, pout), (5, 2, 0.5, 0, pout), (5, 0, 1.5, 0, pout), (5, 0, 0.5, 2, pout), (5, 0, 0.5, 0, None)):
        with pytest.raises(ValueError):
            _lib.check(lib.smesh_face_graph_propagate(graph._h, prow, _lib.MEM_HOST, C, None, _lib.MEM_HOST, mode, 1, alpha, 0.9, out_mode, 0.9,
                                                      po, None, None, _lib.MEM_HOST))
    w = np.zeros(len(nbr), np.float32)
    for power in (0, 17):
        with pytest.raises(ValueError):
            _lib.check(lib.smesh_face_graph_normal_weights(graph._h, faces.ctypes.data_as(ctypes.c_void_p), vertices.ctypes.data_as(ctypes.c_void_p),
                                                           _lib.MEM_HOST, power, 1, w.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
    bad = faces.copy()
    bad[5, 2] = V
    with pytest.raises(ValueError):                                              # faces that are not the graph's: an index out of range
        _lib.check(lib.smesh_face_graph_normal_weights(graph._h, bad.ctypes.data_as(ctypes.c_void_p), vertices.ctypes.data_as(ctypes.c_void_p),
                                                       _lib.MEM_HOST, 4, 1, w.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
    agg = sm.fusion.MeshAggregator(F + 4, 5)
    with pytest.raises(ValueError):                                              # P != F, at the library
        _lib.check(lib.smesh_aggregator_face_propagate(agg._h, graph._h, None, _lib.MEM_HOST, 0, 1, 0.5, 0.9, 0, 0.9, pout, None, None, _lib.MEM_HOST))
