"""Segments of a labelled mesh on the GPU (include/smesh_face_segments.h, fusion.FaceGraph.segments, fusion.FaceSegments) against
tests/face_segments_ref.py, a flood fill in ascending face order.  Every result is an integer (or a row passed through), so every
comparison is exact; the reference of every comparison is computed on the host, never by the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import face_graph_ref as gref
import face_segments_ref as ref
import test_gpu_face_graph as tgf

pytestmark = pytest.mark.gpu

THRESHOLD = 0.9
ISLAND = 18                                       # the label of the stamped islands; the blocks use 0 .. 17
ISLANDS = ((2, 1, 1), (5, 2, 2), (10, 1, 7), (13, 3, 8), (18, 2, 9))      # (quad row i, first quad j, faces)


# ---- meshes (computed once; nobody writes to them) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip_case():
    """4000 x 1 quads: 8 000 faces in one chain, the smallest shape whose diameter is its face count."""
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(4000, 1)
    faces = np.ascontiguousarray(mesh.faces, np.int32)
    assert faces.shape == (8000, 3)
    case = tgf._case(faces, mesh.vertices.astype(np.float32).copy())
    assert np.diff(case[3].astype(np.int64)).max() == 2                      # a chain
    return case


@functools.lru_cache(maxsize=None)
def islands_case():
    """300 triangles that share nothing: a graph without entries, over two workgroups."""
    faces = np.arange(900, dtype=np.int32).reshape(300, 3)
    case = tgf._case(faces, np.random.default_rng(5).random((900, 3), dtype=np.float32))
    assert len(case[4]) == 0
    return case


def tiny_case(F):
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    return tgf._case(faces, np.zeros((3 * F, 3), np.float32))


CASES = {"grid": tgf.grid_case, "soup": tgf.soup_case, "strip": strip_case, "isolated": islands_case}


# ---- label patterns ------------------------------------------------------------------------------------------------------------
def quads(a, b, fn):
    """int32 [2 a b]: fn(i, j) per quad of grid_mesh(a, b), for both of its faces."""
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    return np.repeat(np.asarray(fn(i, j), np.int32).reshape(-1), 2)


def serpentine(a, b):
    """Label 1 winds through the grid between walls of label 0: every even quad row is corridor, every odd one a wall with one gap
    at alternating ends, so the corridor is ONE segment whose diameter is of the order of the face count."""
    def fn(i, j):
        gap = np.where((i // 2) % 2 == 0, b - 1, 0)
        return ((i % 2 == 0) | (j == gap)).astype(np.int32)
    return quads(a, b, fn)


def blocks(a, b, side=8, K=19):
    return quads(a, b, lambda i, j: ((i // side) * 7 + (j // side) * 3) % K)


def stamped(a, b):
    """8 x 8 blocks of 18 labels with islands of 1, 2, 7, 8 and 9 faces of label ISLAND: consecutive faces of one quad row form a path."""
    labels = blocks(a, b, 8, 18)
    for i, j, n in ISLANDS:
        first = 2 * (i * b + j)
        assert j * 2 + n <= 2 * b
        labels[first:first + n] = ISLAND
    return labels


def random_labels(seed, F, K):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, K, F).astype(np.int32)
    labels[rng.random(F) < 0.1] = -1
    return labels


@functools.lru_cache(maxsize=None)
def pattern(case, name):
    F = len(CASES[case]()[0])
    a, b = {"grid": (40, 30), "strip": (4000, 1)}.get(case, (0, 0))
    if name == "constant":
        labels = np.full(F, 5, np.int32)
    elif name == "none":
        labels = np.full(F, -1, np.int32)
    elif name == "negative":                                                 # other negative values are don't care too
        labels = np.where(np.arange(F) % 3 == 0, -7, 4).astype(np.int32)
    elif name == "big":                                                      # 2^31 - 1 is a label
        labels = np.where(np.arange(F) % 5 < 3, 2 ** 31 - 1, 0).astype(np.int32)
    elif name == "stripes":
        labels = quads(a, b, lambda i, j: i % 2)
    elif name == "blocks":
        labels = blocks(a, b)
    elif name == "serpentine":
        labels = serpentine(a, b)
    elif name == "stamped":
        labels = stamped(a, b)
    elif name in ("random2", "random19"):
        labels = random_labels(len(case) + int(name[6:]), F, int(name[6:]))
    else:
        raise KeyError(name)
    assert labels.shape == (F,) and labels.dtype == np.int32
    labels.setflags(write=False)
    return labels


@functools.lru_cache(maxsize=None)
def entry_weights(case, kind):
    """(weights float32[nnz], min_weight)."""
    faces, vertices, V, offsets, nbr = CASES[case]()
    rng = np.random.default_rng(77)
    if kind == "normal":
        w, min_weight = gref.normal_weights(offsets, nbr, vertices, faces), 0.5
    elif kind == "asymmetric":                                               # every entry on its own: most edges pass one way only or not at all
        w, min_weight = rng.random(len(nbr), dtype=np.float32), 0.6
    elif kind == "nan":
        w, min_weight = rng.random(len(nbr), dtype=np.float32), 0.3
        w[rng.random(len(nbr)) < 0.3] = np.nan
    else:
        raise KeyError(kind)
    w.setflags(write=False)
    return w, min_weight


@functools.lru_cache(maxsize=None)
def expected(case, name, kind=None):
    """The reference's (ids, first_face, label, size) -- computed once and shared."""
    faces, vertices, V, offsets, nbr = CASES[case]()
    w, min_weight = entry_weights(case, kind) if kind else (None, None)
    out = ref.segments(offsets, nbr, pattern(case, name), w, min_weight)
    for a in out:
        a.setflags(write=False)
    return out


def special_rows(rng, F, C):
    """float32 [F,C] rows that must pass through bit for bit: -0.0, subnormals, ordinary values."""
    rows = rng.random((F, C), dtype=np.float32)
    rows[rng.random((F, C)) < 0.1] = np.float32(-0.0)
    rows[rng.random((F, C)) < 0.1] = np.float32(1e-42)
    if F:
        rows[0, 0], rows[F - 1, C - 1] = np.float32(-0.0), np.float32(1.4e-45)
    return rows


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_segments(seg, labels, want, min_faces_list=(0, 1, 8), class_counts=(19,), seed=0):
    """Everything a FaceSegments gives against the reference `want` of `labels`."""
    from semantic_meshes_amd.device import to_device
    ids, first, label, size = want
    F = len(labels)
    assert (seg.num_faces, seg.count, seg.num_labelled) == (F, len(first), int((labels >= 0).sum()))
    for got, dev, ref_array, dtype in ((seg.ids(), seg.ids_device(), ids, np.int32), (seg.first_faces(), seg.first_faces_device(), first, np.uint32),
                                       (seg.labels(), seg.labels_device(), label, np.int32), (seg.sizes(), seg.sizes_device(), size, np.uint32)):
        assert got.dtype == dtype and dev.dtype == dtype and got.shape == ref_array.shape == dev.shape
        assert np.array_equal(got, ref_array) and np.array_equal(dev.numpy(), ref_array)
    rng = np.random.default_rng(900 + seed)
    for min_faces in min_faces_list:
        out, faces_gone, segs_gone = ref.despeckle_labels(labels, ids, size, min_faces)
        got, n1, n2 = seg.despeckle_labels(min_faces, return_removed=True)
        dev, m1, m2 = seg.despeckle_labels_device(min_faces, return_removed=True)
        assert got.dtype == np.int32 and np.array_equal(got, out) and np.array_equal(dev.numpy(), out)
        assert (n1, n2) == (faces_gone, segs_gone) == (m1, m2)
        assert np.array_equal(seg.despeckle_labels(min_faces), out)
        if min_faces <= 1:
            assert (faces_gone, segs_gone) == (0, 0)
        for C in class_counts:
            rows = special_rows(rng, F, C)
            before = rows.copy()
            want_rows = ref.despeckle_rows(rows, labels, ids, size, min_faces)
            d_rows = to_device(rows)
            for source in (rows, d_rows):
                got = seg.despeckle_sums(source, min_faces)
                assert got.dtype == np.float32 and got.shape == (F, C) and np.array_equal(u32(got), u32(want_rows))
                assert np.array_equal(u32(seg.despeckle_sums_device(source, min_faces).numpy()), u32(want_rows))
            assert np.array_equal(u32(rows), u32(before)) and np.array_equal(u32(d_rows.numpy()), u32(before))


# ---- 1. labels in, on every mesh -----------------------------------------------------------------------------------------------
PATTERNS = [("grid", n) for n in ("constant", "none", "negative", "big", "stripes", "blocks", "serpentine", "stamped", "random2", "random19")] + \
           [("strip", n) for n in ("constant", "stripes", "random2", "negative")] + \
           [("soup", n) for n in ("constant", "random2", "random19")] + \
           [("isolated", n) for n in ("constant", "random2", "none")]


@pytest.mark.parametrize("case,name", PATTERNS)
def test_segments_equal_the_flood_fill(sm, case, name):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = CASES[case]()
    labels = pattern(case, name)
    want = expected(case, name)
    graph = sm.fusion.FaceGraph(faces, V)
    d_labels = to_device(labels)
    first = graph.segments(labels)
    check_segments(first, labels, want, class_counts=(19, 40) if case == "grid" else (19,), seed=len(name))
    again = graph.segments(d_labels)                                         # device labels; and a second call: equal bits
    for a, b in ((first.ids(), again.ids()), (first.first_faces(), again.first_faces()), (first.labels(), again.labels()),
                 (first.sizes(), again.sizes())):
        assert np.array_equal(a, b)
    assert np.array_equal(again.ids(), want[0]) and again.count == len(want[1])
    assert np.array_equal(graph.segments(labels.astype(np.int64)).ids(), want[0])      # any integer dtype on the host
    assert np.array_equal(d_labels.numpy(), labels)                          # inputs are unchanged


def test_the_patterns_are_what_they_are_for():
    """On the reference alone: the structured patterns have the properties the random ones lack."""
    ids, first, label, size = expected("grid", "constant")
    assert len(first) == 1 and size[0] == 2400
    assert len(expected("grid", "none")[1]) == 0
    ids, first, label, size = expected("grid", "random2")
    assert len(first) > 300 and size.max() < 100                             # hundreds of small segments: not enough on their own
    ids, first, label, size = expected("grid", "stripes")
    assert len(first) == 40 and (size == 60).all()                           # one quad wide
    ids, first, label, size = expected("grid", "serpentine")
    assert (label == 1).sum() == 1 and size[label == 1][0] > 1200            # the corridor is one segment, half the mesh long
    ids, first, label, size = expected("strip", "constant")
    assert len(first) == 1 and size[0] == 8000
    ids, first, label, size = expected("grid", "big")
    assert (label == 2 ** 31 - 1).any()
    ids, first, label, size = expected("isolated", "constant")
    assert len(first) == 300 and (size == 1).all()
    # the stamped islands: with min_faces = 8 those of 1, 2 and 7 faces go, those of 8 and 9 stay, and so does every block
    labels = pattern("grid", "stamped")
    ids, first, label, size = expected("grid", "stamped")
    assert sorted(size[label == ISLAND].tolist()) == [1, 2, 7, 8, 9]
    out, faces_gone, segs_gone = ref.despeckle_labels(labels, ids, size, 8)
    assert (faces_gone, segs_gone) == (10, 3) and (out[labels != ISLAND] == labels[labels != ISLAND]).all()
    for i, j, n in ISLANDS:
        f = 2 * (i * 30 + j)
        assert (out[f:f + n] == (ISLAND if n >= 8 else -1)).all()


# ---- 2. weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name,kind", [("grid", "constant", "normal"), ("grid", "blocks", "normal"), ("grid", "constant", "asymmetric"),
                                            ("grid", "blocks", "asymmetric"), ("grid", "constant", "nan"), ("soup", "random2", "asymmetric"),
                                            ("soup", "constant", "nan"), ("strip", "constant", "asymmetric"), ("soup", "random2", "normal")])
def test_weighted_segments_equal_the_flood_fill(sm, case, name, kind):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = CASES[case]()
    labels = pattern(case, name)
    w, min_weight = entry_weights(case, kind)
    want = expected(case, name, kind)
    graph = sm.fusion.FaceGraph(faces, V)
    d_w = graph.normal_weights(vertices) if kind == "normal" else to_device(w)
    assert np.array_equal(u32(d_w.numpy()), u32(w))
    check_segments(graph.segments(labels, weights=w, min_weight=min_weight), labels, want, min_faces_list=(8,), seed=3)
    seg = graph.segments(to_device(labels), weights=d_w, min_weight=min_weight)
    assert np.array_equal(seg.ids(), want[0]) and np.array_equal(seg.sizes(), want[3])
    assert np.array_equal(u32(d_w.numpy()), u32(w))
    with pytest.raises(ValueError):
        graph.segments(labels, weights=d_w)


def test_the_weights_are_what_they_are_for():
    """On the reference alone."""
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    # the crease along x = 0 cuts the constant mesh: no segment has faces on both sides
    ids = expected("grid", "constant", "normal")[0]
    left = np.repeat(np.arange(40) < 20, 60)                                 # quad rows i < 20 lie at x < 0
    assert len(expected("grid", "constant", "normal")[1]) >= 2 and not set(ids[left].tolist()) & set(ids[~left].tolist())
    # asymmetric weights: some edges link although only one direction passes, and dropping that rule would change the answer
    w, min_weight = entry_weights("grid", "asymmetric")
    f, g, ok = ref.link_mask(offsets, nbr, pattern("grid", "constant"), w, min_weight)
    passing = set(zip(f[ok].tolist(), g[ok].tolist()))
    one_way = [(a, b) for a, b in passing if (b, a) not in passing]
    assert len(one_way) > 100 and any(a < b for a, b in one_way) and any(a > b for a, b in one_way)
    both = np.array([(b, a) in passing for a, b in zip(f.tolist(), g.tolist())]) & ok
    w_both = np.where(both, np.float32(1), np.float32(0))
    assert len(ref.segments(offsets, nbr, pattern("grid", "constant"), w_both, 0.5)[1]) != len(expected("grid", "constant", "asymmetric")[1])
    w, _ = entry_weights("grid", "nan")
    assert np.isnan(w).any()


# ---- 3. rows and aggregators as the source -------------------------------------------------------------------------------------
def rows_of(labels, C, seed):
    """float32 [F,C]: the label's class dominates; a tenth of the labelled faces stay below the threshold, unlabelled faces are zero."""
    rng = np.random.default_rng(seed)
    F = len(labels)
    rows = (rng.random((F, C), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    sel = labels >= 0
    rows[np.flatnonzero(sel), labels[sel]] += np.float32(1.0)
    rows /= rows.sum(axis=1, keepdims=True)
    rows[rng.random(F) < 0.1] *= np.float32(0.3)
    rows[~sel] = 0.0
    return rows


@pytest.mark.parametrize("C", [19, 40])
def test_rows_as_the_source_and_the_fill_that_follows(sm, C):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    rows = rows_of(pattern("grid", "stamped"), C, 40 + C)
    before = rows.copy()
    labels = ref.row_labels(rows, THRESHOLD)
    assert (labels == -1).sum() > 100 and (labels == ISLAND).any()
    want = ref.segments(offsets, nbr, labels)
    graph = sm.fusion.FaceGraph(faces, V)
    d_rows = to_device(rows)
    for source in (rows, d_rows):
        check_segments(graph.segments(source, dont_care_threshold=THRESHOLD), labels, want, min_faces_list=(8,), class_counts=(C,), seed=C)
    assert graph.segments(rows, dont_care_threshold=0.2).num_labelled == int((ref.row_labels(rows, 0.2) >= 0).sum()) > (labels >= 0).sum()
    # end to end: the islands go, their surroundings grow back in -- the reference chain, bit for bit
    seg = graph.segments(d_rows, dont_care_threshold=THRESHOLD)
    cleaned = ref.despeckle_rows(rows, labels, want[0], want[3], 8)
    assert (u32(cleaned) != u32(rows)).any()
    x, tot = gref.propagate(offsets, nbr, cleaned, 4, gref.FILL, observed_threshold=THRESHOLD)
    want_labels = gref.finish(x, tot, THRESHOLD)[0]
    got = graph.fill_labels(seg.despeckle_sums_device(d_rows, 8), 4, THRESHOLD, None, THRESHOLD)
    assert np.array_equal(got, want_labels)
    tgf.assert_bits(graph.fill_sums(seg.despeckle_sums(rows, 8), 4, THRESHOLD), x)
    for i, j, n in ISLANDS[:3]:                                              # the small islands took their block's label
        f = 2 * (i * 30 + j)
        assert (want_labels[f:f + n] != ISLAND).all()
    assert np.array_equal(u32(rows), u32(before)) and np.array_equal(u32(d_rows.numpy()), u32(before))


@pytest.mark.parametrize("kind", ["sum", "mul"])
def test_from_an_aggregator(sm, kind):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(40, 20)
    F, C = len(mesh.faces), 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    graph = sm.fusion.FaceGraph.from_mesh(mesh)
    offsets, nbr = gref.adjacency(mesh.faces, len(mesh.vertices))
    agg = sm.fusion.MeshAggregator(F, C, kind)
    tgf._fuse(sm, agg, sm.render.triangles(mesh), cams, C)
    seg = graph.segments(agg, dont_care_threshold=THRESHOLD)                 # deferred views are handed over first, as get() does
    assert not agg._pending
    raw = agg.get_raw().copy()
    rows = agg.get()
    labels = ref.row_labels(rows, THRESHOLD)
    assert np.array_equal(labels, agg.labels(THRESHOLD)) and (labels >= 0).mean() > 0.3
    assert kind == "mul" or (labels < 0).any()                                # (Mul renormalises every row: all of its faces are labelled)
    want = ref.segments(offsets, nbr, labels)
    assert len(want[1]) > 10
    min_faces = int(np.sort(want[3])[len(want[3]) // 2]) + 1                  # removes about half of the segments
    check_segments(seg, labels, want, min_faces_list=(min_faces,), seed=7)
    assert np.array_equal(graph.segments(agg.labels_device(THRESHOLD)).ids(), want[0])
    assert np.array_equal(graph.segments(rows, dont_care_threshold=THRESHOLD).ids(), want[0])      # exactly what its get() rows give
    cleaned = ref.despeckle_rows(rows, labels, want[0], want[3], min_faces)
    assert (u32(cleaned) != u32(rows)).any()
    assert np.array_equal(u32(seg.despeckle_sums(agg, min_faces)), u32(cleaned))
    assert np.array_equal(u32(seg.despeckle_sums_device(agg, min_faces).numpy()), u32(cleaned))
    w = graph.normal_weights(mesh.vertices)
    want_w = ref.segments(offsets, nbr, labels, gref.normal_weights(offsets, nbr, mesh.vertices, mesh.faces), 0.999)
    got_w = graph.segments(agg, weights=w, min_weight=0.999, dont_care_threshold=THRESHOLD)
    assert np.array_equal(got_w.ids(), want_w[0]) and got_w.count == len(want_w[1]) >= len(want[1])
    # the workflow of the README, against the reference chain
    x, tot = gref.propagate(offsets, nbr, cleaned, 8, gref.FILL, observed_threshold=THRESHOLD)
    clean = graph.fill_labels_device(seg.despeckle_sums_device(agg, min_faces), iterations=8)
    assert np.array_equal(clean.numpy(), gref.finish(x, tot, THRESHOLD)[0])
    assert np.array_equal(u32(agg.get_raw()), u32(raw)) and np.array_equal(u32(agg.get()), u32(rows))      # the accumulator is untouched
    with pytest.raises(ValueError):
        graph.segments(sm.fusion.MeshAggregator(F + 1, C, kind))             # P != F
    with pytest.raises(ValueError):
        seg.despeckle_sums(sm.fusion.MeshAggregator(F + 1, C, kind), 3)


# ---- 4. one face, no face ------------------------------------------------------------------------------------------------------
def test_one_face_and_no_face(sm):
    faces, vertices, V, offsets, nbr = tiny_case(1)
    graph = sm.fusion.FaceGraph(faces, V)
    for value, want in ((6, ([0], [0], [6], [1])), (-1, ([-1], [], [], []))):
        seg = graph.segments(np.array([value], np.int32))
        assert (seg.ids().tolist(), seg.first_faces().tolist(), seg.labels().tolist(), seg.sizes().tolist()) == want
        assert (seg.num_faces, seg.count, seg.num_labelled) == (1, len(want[1]), int(value >= 0))
        out, n1, n2 = seg.despeckle_labels(2, return_removed=True)
        assert out.tolist() == [-1] and (n1, n2) == (int(value >= 0), int(value >= 0))
        assert seg.despeckle_labels(1).tolist() == [value if value >= 0 else -1]
        rows = np.array([[0.5, -0.0, 1e-42]], np.float32)
        assert np.array_equal(u32(seg.despeckle_sums(rows, 2)), u32(rows if value < 0 else 0 * np.abs(rows)))
        assert np.array_equal(u32(seg.despeckle_sums(rows, 1)), u32(rows))
    faces, vertices, V, offsets, nbr = tiny_case(0)
    graph = sm.fusion.FaceGraph(faces, 0)
    seg = graph.segments(np.zeros(0, np.int32))
    assert (seg.num_faces, seg.count, seg.num_labelled) == (0, 0, 0)
    assert len(seg.ids()) == len(seg.first_faces()) == len(seg.labels()) == len(seg.sizes()) == 0
    out, n1, n2 = seg.despeckle_labels(3, return_removed=True)
    assert len(out) == 0 and (n1, n2) == (0, 0)
    assert seg.despeckle_sums(np.zeros((0, 5), np.float32), 3).shape == (0, 5)
    assert seg.ids_device().shape == (0,) and seg.despeckle_labels_device(3).shape == (0,)


# ---- 5. errors at the library --------------------------------------------------------------------------------------------------
def test_errors_are_value_errors(sm):
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    F = len(faces)
    graph = sm.fusion.FaceGraph(faces, V)
    labels = pattern("grid", "blocks")
    with pytest.raises(ValueError):
        graph.segments(to_device(labels.astype(np.int64)))                   # a device array must be int32
    with pytest.raises(ValueError):
        graph.segments(to_device(labels[:-1].copy()))
    with pytest.raises(ValueError):
        graph.segments(labels, weights=to_device(np.zeros(len(nbr) + 1, np.float32)), min_weight=0.5)
    lib = _lib.lib()
    plab = labels.ctypes.data_as(ctypes.c_void_p)
    w = np.ones(len(nbr), np.float32)
    h = ctypes.c_void_p()
    for g, pl, lmem, pw, wmem, out in ((None, plab, _lib.MEM_HOST, None, _lib.MEM_HOST, ctypes.byref(h)),      # no graph
                                       (graph._h, None, _lib.MEM_HOST, None, _lib.MEM_HOST, ctypes.byref(h)),   # no labels
                                       (graph._h, plab, 7, None, _lib.MEM_HOST, ctypes.byref(h)),               # bad memory kinds
                                       (graph._h, plab, _lib.MEM_HOST, w.ctypes.data_as(ctypes.c_void_p), 7, ctypes.byref(h)),
                                       (graph._h, plab, _lib.MEM_HOST, None, _lib.MEM_HOST, None)):             # no out
        with pytest.raises(ValueError):
            _lib.check(lib.smesh_face_segments_create(g, pl, lmem, pw, wmem, 0.5, out))
        assert not h.value
    agg = sm.fusion.MeshAggregator(F + 4, 5)
    with pytest.raises(ValueError):                                          # P != F
        _lib.check(lib.smesh_aggregator_face_segments(agg._h, graph._h, 0.9, None, _lib.MEM_HOST, 0.0, ctypes.byref(h)))
    assert not h.value
    with pytest.raises(ValueError):
        _lib.check(lib.smesh_aggregator_face_segments(None, graph._h, 0.9, None, _lib.MEM_HOST, 0.0, ctypes.byref(h)))
    seg = graph.segments(labels)
    out = np.zeros(F, np.int32)
    rows, out_rows = np.zeros((F, 5), np.float32), np.zeros((F, 5), np.float32)
    pout, prow, porow = (a.ctypes.data_as(ctypes.c_void_p) for a in (out, rows, out_rows))
    for call in (lambda: lib.smesh_face_segments_despeckle_labels(seg._h, 8, None, _lib.MEM_HOST, None, None),
                 lambda: lib.smesh_face_segments_despeckle_labels(seg._h, 8, pout, 7, None, None),
                 lambda: lib.smesh_face_segments_despeckle_labels(None, 8, pout, _lib.MEM_HOST, None, None),
                 lambda: lib.smesh_face_segments_despeckle_rows(seg._h, 8, prow, _lib.MEM_HOST, 0, porow, _lib.MEM_HOST),      # C == 0
                 lambda: lib.smesh_face_segments_despeckle_rows(seg._h, 8, None, _lib.MEM_HOST, 5, porow, _lib.MEM_HOST),
                 lambda: lib.smesh_face_segments_despeckle_rows(seg._h, 8, prow, _lib.MEM_HOST, 5, None, _lib.MEM_HOST),
                 lambda: lib.smesh_face_segments_despeckle_rows(seg._h, 8, prow, 7, 5, porow, _lib.MEM_HOST),
                 lambda: lib.smesh_face_segments_despeckle_rows(seg._h, 8, prow, _lib.MEM_HOST, 5, porow, 7),
                 lambda: lib.smesh_face_segments_get(seg._h, pout, None, None, None, 7),
                 lambda: lib.smesh_face_segments_get(None, pout, None, None, None, _lib.MEM_HOST),
                 lambda: lib.smesh_face_segments_size(None, None, None, None),
                 lambda: lib.smesh_aggregator_face_segments_despeckle(agg._h, seg._h, 8, porow, _lib.MEM_HOST),                # P != F
                 lambda: lib.smesh_aggregator_face_segments_despeckle(None, seg._h, 8, porow, _lib.MEM_HOST)):
        with pytest.raises(ValueError):
            _lib.check(call())
    # every out pointer of get() and size() may be NULL; the removed counts are optional
    _lib.check(lib.smesh_face_segments_get(seg._h, None, None, None, None, _lib.MEM_HOST))
    _lib.check(lib.smesh_face_segments_size(seg._h, None, None, None))
    _lib.check(lib.smesh_face_segments_despeckle_labels(seg._h, 8, pout, _lib.MEM_HOST, None, None))
    assert np.array_equal(out, ref.despeckle_labels(labels, *[expected("grid", "blocks")[k] for k in (0, 3)], 8)[0])
    assert lib.smesh_face_segments_destroy(None) == 0
