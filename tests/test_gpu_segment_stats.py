"""Fused rows and areas pooled over segments on the GPU (include/smesh_segment_stats.h, fusion.FaceGraph.face_areas,
fusion.FaceSegments.members / pool* / areas / despeckle_*_by) against tests/segment_stats_ref.py.  The header defines every result to
the bit -- one float32 operation after another in a stated order -- so every comparison is exact: that tolerance follows from the
rule, it was not measured.  The reference of every comparison is computed on the host, never by the code under test; the segment ids
come from the flood fill of tests/face_segments_ref.py."""
import ctypes
import functools

import numpy as np
import pytest

import face_graph_ref as gref
import face_segments_ref as sref
import mesh_graph_scale_cases as cases
import segment_stats_ref as ref
import test_gpu_face_graph as tgf
import test_gpu_face_segments as tfs

pytestmark = pytest.mark.gpu

THRESHOLD = 0.9
LADDER_RUNS = (1, -100, 255, 256, 257, 511, 512, 513, 65537)     # faces per label run of the strip; negative: a run of unlabelled faces
LADDER_CLASSES = (1, 19, 40, 65)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    diff = u32(got) != u32(want)
    assert not diff.any(), "%d of %d elements differ" % (int(diff.sum()), got.size)


def wide_rows(rng, F, C):
    """Non-negative float32 rows whose magnitudes span 2^-20 .. 2^20: a sum of them depends on the order of its additions."""
    return (rng.random((F, C), dtype=np.float32) * np.float32(2.0) ** rng.integers(-20, 21, (F, C)).astype(np.float32)).astype(np.float32)


def check_members(seg, ids, count):
    want_offsets, want_members = ref.members(ids, count)
    for offsets, members in (seg.members(), tuple(a.numpy() for a in seg.members_device()), seg.members()):      # (and a second call)
        assert offsets.dtype == np.uint32 and members.dtype == np.uint32
        assert np.array_equal(offsets, want_offsets) and np.array_equal(members, want_members)


# ---- 1. the member table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name", tfs.PATTERNS)
def test_members_equal_the_stable_argsort(sm, case, name):
    faces, vertices, V, offsets, nbr = tfs.CASES[case]()
    ids, first, label, size = tfs.expected(case, name)
    seg = sm.fusion.FaceGraph(faces, V).segments(tfs.pattern(case, name))
    assert seg.count == len(first)
    check_members(seg, ids, len(first))
    assert np.array_equal(np.diff(seg.members()[0].astype(np.int64)), size)


@functools.lru_cache(maxsize=None)
def shuffled_small():
    """A 46 x 45 grid (4 140 faces) in a seeded random face order: its two halves (labels 0 and 1, over 1 500 faces each) interleave
    in face index, 6 % of the faces carry noise labels and 3 % none.  (faces, V, labels, the flood fill's results)."""
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(46, 45)
    rng = np.random.default_rng(4140)
    labels = tfs.quads(46, 45, lambda i, j: (i >= 23).astype(np.int32))
    hit = rng.random(len(labels))
    labels[hit < 0.06] = rng.integers(2, 6, int((hit < 0.06).sum()))
    labels[hit > 0.97] = -1
    perm = rng.permutation(len(labels))
    faces, labels = np.ascontiguousarray(mesh.faces[perm], np.int32), np.ascontiguousarray(labels[perm])
    V = len(mesh.vertices)
    off, nbr = gref.adjacency(faces, V)
    out = sref.segments(off, nbr, labels)
    for a in (faces, labels) + out:
        a.setflags(write=False)
    return faces, V, labels, out


def test_members_of_interleaved_segments(sm):
    faces, V, labels, (ids, first, label, size) = shuffled_small()
    big = np.flatnonzero(size > 256)
    assert len(faces) == 4140 and len(big) >= 2 and len(first) > 100 and (labels < 0).any()
    a, b = (np.flatnonzero(ids == s) for s in big[:2])
    assert a[0] < b[-1] and b[0] < a[-1] and np.abs(np.diff((ids == big[0]).astype(int))).sum() > 500      # interleaved in face index
    seg = sm.fusion.FaceGraph(faces, V).segments(labels)
    check_members(seg, ids, len(first))
    rng = np.random.default_rng(7)
    for C in (3, 8):
        rows = wide_rows(rng, len(faces), C)
        assert_bits(seg.pool_sums(rows), ref.pooled(rows, ids, len(first)))


@pytest.mark.parametrize("bits", [0, 1, 2, 3, 4, 9])
def test_every_sort_digit_width_gives_the_same_table(sm, monkeypatch, bits):
    """SMESH_SEGMENT_SORT_BITS (read at every build, clamped to 1 .. 4): the one-bit split and every digit width, whole passes and a
    narrower last one, on few and on 15 165 segments."""
    monkeypatch.setenv("SMESH_SEGMENT_SORT_BITS", str(bits))
    faces, V, labels, (ids, first, label, size) = shuffled_small()
    check_members(sm.fusion.FaceGraph(faces, V).segments(labels), ids, len(first))
    faces, V, labels, ids, S, size = ladder()
    check_members(sm.fusion.FaceGraph(faces, V).segments(labels), ids, S)
    faces, vertices, V, offsets, nbr = cases.case("shuffled")
    ids, first, label, size = cases.expected("shuffled", "blocks32_noisy")
    assert 2 ** 13 < len(first) <= 2 ** 14                         # 14 bits: 4 + 4 + 4 + 2, 3 x 4 + 2, 7 x 2
    check_members(sm.fusion.FaceGraph(faces, V).segments(cases.labels("shuffled", "blocks32_noisy")), ids, len(first))


@pytest.mark.parametrize("labels", [[-1, -1, -1], [5, -1, -1], [5, -1, 5], [5, 5, 5], [6], [-1], []])
def test_members_of_zero_to_three_segments(sm, labels):
    labels = np.asarray(labels, np.int32)
    F = len(labels)
    faces, vertices, V, offsets, nbr = tfs.tiny_case(F)            # F triangles that share nothing: every labelled face is a segment
    seg = sm.fusion.FaceGraph(faces, V).segments(labels)
    ids = np.where(labels >= 0, np.cumsum(labels >= 0) - 1, -1)
    S = int((labels >= 0).sum())
    assert seg.count == S and np.array_equal(seg.ids(), ids)
    check_members(seg, ids, S)
    rows = np.arange(1, 2 * F + 1, dtype=np.float32).reshape(F, 2)
    w = np.arange(2, F + 2, dtype=np.float32)
    assert_bits(seg.pool_sums(rows), ref.pooled(rows, ids, S))
    assert_bits(seg.pool_sums(rows, face_weights=w), ref.pooled(rows, ids, S, w))
    assert_bits(seg.pooled_face_sums(rows, face_weights=w), ref.pooled_faces(rows, ids, S, w))
    assert np.array_equal(seg.pool_labels(rows), np.ones(S, np.int32))
    assert np.array_equal(seg.pooled_face_labels(rows), np.ones(F, np.int32))
    assert seg.pool_sums_device(rows).shape == (S, 2) and seg.areas(np.ones(F, np.float32)).tolist() == [1.0] * S
    out, n1, n2 = seg.despeckle_labels_by(np.zeros(S, np.float32), 1.0, return_removed=True)
    assert out.tolist() == [-1] * F and (n1, n2) == (S, S)
    assert np.array_equal(seg.despeckle_labels_by(np.ones(S, np.float32), 1.0), np.where(labels >= 0, labels, -1))
    assert_bits(seg.despeckle_sums_by(rows, np.ones(S, np.float32), 1.0), rows)


# ---- 2. the size ladder ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder():
    """One strip of quads whose label runs have LADDER_RUNS faces, in a seeded random face order so that no segment's members are
    consecutive.  (faces, V, labels, ids, count, sizes)."""
    from semantic_meshes_amd import synth
    F = sum(abs(n) for n in LADDER_RUNS)
    assert F % 2 == 0
    mesh = synth.grid_mesh(F // 2, 1)
    assert len(mesh.faces) == F
    labels = np.concatenate([np.full(abs(n), -1 if n < 0 else 3 + k % 2, np.int32) for k, n in enumerate(LADDER_RUNS)])
    perm = np.random.default_rng(65537).permutation(F)
    faces, labels = np.ascontiguousarray(mesh.faces[perm], np.int32), np.ascontiguousarray(labels[perm])
    V = len(mesh.vertices)
    off, nbr = gref.adjacency(faces, V)
    ids, first, label, size = sref.segments(off, nbr, labels)
    assert sorted(size.tolist()) == sorted(n for n in LADDER_RUNS if n > 0)      # the runs are the segments
    for a in (faces, labels, ids, size):
        a.setflags(write=False)
    return faces, V, labels, ids, len(first), size


@functools.lru_cache(maxsize=None)
def ladder_inputs(C):
    """(rows, weights, pooled without weights, pooled with weights)."""
    faces, V, labels, ids, S, size = ladder()
    rng = np.random.default_rng(1000 + C)
    rows = wide_rows(rng, len(faces), C)
    w = (rng.random(len(faces), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    out = (rows, w, ref.pooled(rows, ids, S), ref.pooled(rows, ids, S, w))
    for a in out:
        a.setflags(write=False)
    return out


def test_the_ladder_is_what_it_is_for():
    """On the reference alone: the rule's sum differs from a plain serial sum and from the rule applied to another member order."""
    faces, V, labels, ids, S, size = ladder()
    assert S == 8 and (labels < 0).sum() == 100
    rows, w, pooled, pooled_w = ladder_inputs(19)
    exponent = np.frexp(rows[rows > 0])[1]
    assert exponent.min() < -15 and exponent.max() > 15
    s = int(np.argmax(size))
    assert size[s] == 65537 and -(-65537 // 256) == 257            # 257 partials: one past a 256-wide pass over partials
    mem = np.flatnonzero(ids == s)
    plain = np.add.accumulate(rows[mem], axis=0, dtype=np.float32)[-1]      # (accumulate adds one after another)
    assert (u32(plain) != u32(pooled[s])).any()
    shuffled = rows.copy()
    shuffled[mem] = rows[np.random.default_rng(3).permutation(mem)]
    assert (u32(ref.pooled(shuffled, ids, S)[s]) != u32(pooled[s])).any()
    small = int(np.flatnonzero(size == 256)[0])                    # at most 256 members: the plain ascending sum
    assert np.array_equal(u32(np.add.accumulate(rows[ids == small], axis=0, dtype=np.float32)[-1]), u32(pooled[small]))
    assert (u32(pooled_w) != u32(pooled)).any()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", LADDER_CLASSES)
def test_the_size_ladder(sm, C, weighted):
    from semantic_meshes_amd.device import to_device
    faces, V, labels, ids, S, size = ladder()
    seg = sm.fusion.FaceGraph(faces, V).segments(labels)
    assert seg.count == S and np.array_equal(seg.ids(), ids)
    check_members(seg, ids, S)
    rows, w, pooled, pooled_w = ladder_inputs(C)
    want = pooled_w if weighted else pooled
    d_rows = to_device(rows)
    fw = to_device(w) if weighted else None
    x = rows.copy()
    x[ids >= 0] = want[ids[ids >= 0]]
    want_ann, want_labels = ref.finish(want, ref.ANNOTATIONS, THRESHOLD)
    want_face_ann, want_face_labels = ref.finish(x, ref.ANNOTATIONS, THRESHOLD)
    assert_bits(seg.pool_sums(d_rows, fw), want)
    assert_bits(seg.pool(d_rows, fw, THRESHOLD), want_ann)
    assert np.array_equal(seg.pool_labels(d_rows, fw, THRESHOLD), want_labels)
    assert_bits(seg.pooled_face_sums(d_rows, fw), x)
    assert_bits(seg.pooled_face_annotations(d_rows, fw, THRESHOLD), want_face_ann)
    assert np.array_equal(seg.pooled_face_labels(d_rows, fw, THRESHOLD), want_face_labels)
    assert_bits(seg.pool_sums(rows, w if weighted else None), want)                       # host inputs; and a second call: equal bits
    assert np.array_equal(u32(d_rows.numpy()), u32(rows))                                # inputs are unchanged


# ---- 3. past the sizes where the launches change -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pattern", [("big", "constant"), ("big", "blocks32_noisy"), ("shuffled", "constant"), ("shuffled", "blocks32_noisy")])
def test_at_scale(sm, name, pattern):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = cases.case(name)
    ids, first, label, size = cases.expected(name, pattern)
    assert len(faces) == cases.BIG_F > cases.CAPPED_GRID > cases.SCAN_CHUNK
    seg = sm.fusion.FaceGraph(faces, V).segments(cases.labels(name, pattern))
    assert seg.count == len(first)
    want_offsets, want_members = ref.members(ids, len(first))
    offsets_got, members_got = seg.members()
    assert np.array_equal(offsets_got, want_offsets) and np.array_equal(members_got, want_members)
    rows = cases.rows(19, 19)
    assert_bits(seg.pool_sums(to_device(rows)), ref.pooled(rows, ids, len(first)))


# ---- 4. areas ------------------------------------------------------------------------------------------------------------------
def test_face_and_segment_areas(sm):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    v = vertices.copy()
    v[faces[7][1]] = v[faces[7][0]]                                # face 7 and its neighbours around that vertex lose their area
    want = ref.face_areas(v, faces)
    assert want[7] == 0 and (want > 0).sum() > 2000 and not u32(want[want == 0]).any()
    graph = sm.fusion.FaceGraph(faces, V)
    got = graph.face_areas(v)
    assert_bits(got, want)
    d_area = graph.face_areas_device(to_device(v))
    assert_bits(d_area.numpy(), want)
    labels = tfs.pattern("grid", "stamped")
    ids, first, label, size = tfs.expected("grid", "stamped")
    seg = graph.segments(labels)
    want_areas = ref.areas(want, ids, len(first))
    for a in (seg.areas(got), seg.areas(d_area), seg.areas_device(got).numpy(), seg.areas_device(d_area).numpy()):
        assert_bits(a, want_areas)
    assert_bits(seg.pool_sums(got[:, None])[:, 0], want_areas)
    assert_bits(seg.pool_sums(np.ones((len(faces), 1), np.float32))[:, 0], size.astype(np.float32))      # (small integers add exactly)
    with pytest.raises(ValueError):
        graph.face_areas(v[:-1])


# ---- 5. the despeckle by a measure -----------------------------------------------------------------------------------------------
def test_despeckle_by_a_measure(sm):
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    labels = tfs.pattern("grid", "stamped")
    ids, first, label, size = tfs.expected("grid", "stamped")
    S, F = len(first), len(faces)
    seg = sm.fusion.FaceGraph(faces, V).segments(labels)
    rng = np.random.default_rng(55)
    measure = rng.random(S, dtype=np.float32)
    measure[3] = np.nan
    measure[5] = np.float32(0.5)                                   # >= : equality passes
    rows40, rows19 = tfs.special_rows(rng, F, 40), tfs.special_rows(rng, F, 19)
    for minimum in (0.5, 0.0, float("nan")):
        want, faces_gone, segs_gone = ref.despeckle_labels_by(labels, ids, measure, minimum)
        assert faces_gone >= size[3] and want[ids == 3].max() == -1      # the NaN removes its segment, whatever the minimum
        assert minimum != 0.5 or (want[ids == 5] >= 0).all()
        for m in (measure, to_device(measure)):
            got, n1, n2 = seg.despeckle_labels_by(m, minimum, return_removed=True)
            dev, m1, m2 = seg.despeckle_labels_by_device(m, minimum, return_removed=True)
            assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(dev.numpy(), want)
            assert (n1, n2) == (faces_gone, segs_gone) == (m1, m2)
            assert np.array_equal(seg.despeckle_labels_by(m, minimum), want)
            for rows in (rows40, rows19):
                want_rows = ref.despeckle_rows_by(rows, ids, measure, minimum)
                assert_bits(seg.despeckle_sums_by(rows, m, minimum), want_rows)
                assert_bits(seg.despeckle_sums_by_device(to_device(rows), m, minimum).numpy(), want_rows)
    clean = np.abs(np.nan_to_num(measure))
    out, n1, n2 = seg.despeckle_labels_by(clean, 0, return_removed=True)      # minimum = 0 keeps every labelled face
    assert np.array_equal(out, np.where(labels >= 0, labels, -1)) and (n1, n2) == (0, 0)
    sizes = seg.sizes().astype(np.float32)                         # with the sizes as the measure: the existing despeckle
    for min_faces in (0, 8, 9):
        assert seg.despeckle_labels_by(sizes, min_faces, return_removed=True)[1:] == seg.despeckle_labels(min_faces, return_removed=True)[1:]
        assert np.array_equal(seg.despeckle_labels_by(sizes, min_faces), seg.despeckle_labels(min_faces))
        assert_bits(seg.despeckle_sums_by(rows19, sizes, min_faces), seg.despeckle_sums(rows19, min_faces))
    assert seg.despeckle_labels(8, return_removed=True)[1:] == (10, 3)


# ---- 6. sources ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sum", "mul"])
def test_from_an_aggregator(sm, kind):
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.device import to_device
    mesh = synth.grid_mesh(40, 20)
    F, C = len(mesh.faces), 19
    cams = [synth.ring_camera(k, 3, 320, 240) for k in range(3)]
    graph = sm.fusion.FaceGraph.from_mesh(mesh)
    agg = sm.fusion.MeshAggregator(F, C, kind)
    tgf._fuse(sm, agg, sm.render.triangles(mesh), cams, C)
    v = mesh.vertices.astype(np.float32).copy()
    v[:, 2] += np.float32(0.8) * np.abs(v[:, 0])                   # bent along x = 0: the crease cuts the README's patches
    seg = graph.segments(np.zeros(F, np.int32), weights=graph.normal_weights(v), min_weight=0.95)
    first = seg.pool_sums(agg)                                     # deferred views are handed over first, as get() does
    assert not agg._pending
    raw, rows = agg.get_raw().copy(), agg.get()
    ids, S = seg.ids(), seg.count
    off, nbr = gref.adjacency(mesh.faces, len(v))
    assert np.array_equal(ids, sref.segments(off, nbr, np.zeros(F, np.int32), gref.normal_weights(off, nbr, v, mesh.faces), 0.95)[0])
    assert S >= 2 and seg.sizes().max() > 256                      # (more than one chunk)
    area = graph.face_areas(v)
    measure, minimum = np.arange(S, dtype=np.float32), 1.0         # segment 0 goes
    want, want_w = ref.pooled(rows, ids, S), ref.pooled(rows, ids, S, area)
    assert_bits(first, want)
    d_rows, d_area = to_device(rows), to_device(area)
    for source in (agg, rows, d_rows):
        assert_bits(seg.pool_sums(source), want)
        assert_bits(seg.pool_sums_device(source).numpy(), want)
        for fw in (area, d_area):
            assert_bits(seg.pool_sums(source, fw), want_w)
        assert_bits(seg.pool(source, area, THRESHOLD), ref.finish(want_w, ref.ANNOTATIONS, THRESHOLD)[0])
        assert_bits(seg.pool_device(source, d_area, THRESHOLD).numpy(), ref.finish(want_w, ref.ANNOTATIONS, THRESHOLD)[0])
        assert np.array_equal(seg.pool_labels(source), ref.finish(want, ref.ANNOTATIONS, 0.9)[1])
        assert np.array_equal(seg.pool_labels_device(source).numpy(), ref.finish(want, ref.ANNOTATIONS, 0.9)[1])
        x = ref.pooled_faces(rows, ids, S)
        assert_bits(seg.pooled_face_sums(source), x)
        assert_bits(seg.pooled_face_sums_device(source).numpy(), x)
        assert_bits(seg.pooled_face_annotations(source, None, THRESHOLD), ref.finish(x, ref.ANNOTATIONS, THRESHOLD)[0])
        assert_bits(seg.pooled_face_annotations_device(source, None, THRESHOLD).numpy(), ref.finish(x, ref.ANNOTATIONS, THRESHOLD)[0])
        assert np.array_equal(seg.pooled_face_labels(source), ref.finish(x, ref.ANNOTATIONS, 0.9)[1])
        assert np.array_equal(seg.pooled_face_labels_device(source).numpy(), ref.finish(x, ref.ANNOTATIONS, 0.9)[1])
        assert_bits(seg.despeckle_sums_by(source, measure, minimum), ref.despeckle_rows_by(rows, ids, measure, minimum))
        assert_bits(seg.despeckle_sums_by_device(source, to_device(measure), minimum).numpy(), ref.despeckle_rows_by(rows, ids, measure, minimum))
    assert (ref.despeckle_rows_by(rows, ids, measure, minimum) != rows).any()
    assert_bits(seg.areas(d_area), ref.areas(area, ids, S))
    assert np.array_equal(u32(agg.get_raw()), u32(raw)) and np.array_equal(u32(agg.get()), u32(rows))      # the accumulator is untouched
    for call in (seg.pool_sums, seg.pooled_face_labels, lambda a: seg.despeckle_sums_by(a, measure, 1.0)):
        with pytest.raises(ValueError):
            call(sm.fusion.MeshAggregator(F + 1, C, kind))           # P != F
    other = sm.fusion.MeshAggregator(F, C, kind)
    other.device = 1                                               # (an aggregator that says it lives elsewhere)
    with pytest.raises(ValueError):
        seg.pool_sums(other)
    other.device = 0


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_are_value_errors(sm):
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.device import to_device
    faces, vertices, V, offsets, nbr = tgf.grid_case()
    F = len(faces)
    graph = sm.fusion.FaceGraph(faces, V)
    seg = graph.segments(tfs.pattern("grid", "blocks"))
    S = seg.count
    rows, w, measure = np.zeros((F, 5), np.float32), np.ones(F, np.float32), np.ones(S, np.float32)
    for bad in (to_device(np.zeros((F, 5), np.float64)), to_device(np.zeros((F + 1, 5), np.float32)), np.zeros((F, 5), np.float64), np.zeros(F, np.float32)):
        with pytest.raises(ValueError):
            seg.pool_sums(bad)
        with pytest.raises(ValueError):
            seg.pooled_face_labels_device(bad)
        with pytest.raises(ValueError):
            seg.despeckle_sums_by(bad, measure, 0.5)
    for bad in (to_device(np.ones(F, np.float64)), to_device(np.ones(F + 1, np.float32)), np.ones(F - 1, np.float32), np.ones(F, np.int32)):
        with pytest.raises(ValueError):
            seg.pool_sums(rows, face_weights=bad)
        with pytest.raises(ValueError):
            seg.areas(bad)
    for bad in (to_device(np.ones(S, np.float64)), to_device(np.ones(S + 1, np.float32)), np.ones(S - 1, np.float32), None):
        with pytest.raises(ValueError):
            seg.despeckle_labels_by(bad, 0.5)
    for bad in ("1", None, [1.0], True):
        with pytest.raises(ValueError):
            seg.despeckle_labels_by(measure, bad)
    elsewhere = to_device(w)
    elsewhere.device = 1                                           # (a device array that says it lives elsewhere)
    with pytest.raises(ValueError):
        seg.pool_sums(rows, face_weights=elsewhere)
    elsewhere.device = 0
    lib = _lib.lib()
    out_rows, out_labels, out_faces = np.zeros((S, 5), np.float32), np.zeros(S, np.int32), np.zeros(F, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    H, SUMS = _lib.MEM_HOST, _lib.VTX_SUMS
    for call in (lambda: lib.smesh_segment_stats_pool(None, ptr(rows), H, 5, None, H, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_segment_stats_pool(seg._h, None, H, 5, None, H, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), 7, 5, None, H, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 0, None, H, SUMS, 0.9, ptr(out_rows), None, H),      # C == 0
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 5, ptr(w), 7, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 5, None, H, 5, 0.9, ptr(out_rows), None, H),         # a bad mode
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 5, None, H, SUMS, 0.9, None, None, H),               # no output
                 lambda: lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 5, None, H, SUMS, 0.9, ptr(out_rows), None, 7),
                 lambda: lib.smesh_segment_stats_pool_faces(seg._h, ptr(rows), H, 5, None, H, SUMS, 0.9, None, None, H),
                 lambda: lib.smesh_aggregator_segment_stats_pool(None, seg._h, None, H, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_aggregator_segment_stats_pool_faces(None, seg._h, None, H, SUMS, 0.9, ptr(out_rows), None, H),
                 lambda: lib.smesh_segment_stats_members(None, None, None, H),
                 lambda: lib.smesh_segment_stats_members(seg._h, None, None, 7),
                 lambda: lib.smesh_segment_stats_despeckle_labels(None, ptr(measure), H, 0.5, ptr(out_faces), H, None, None),
                 lambda: lib.smesh_segment_stats_despeckle_labels(seg._h, None, H, 0.5, ptr(out_faces), H, None, None),
                 lambda: lib.smesh_segment_stats_despeckle_labels(seg._h, ptr(measure), 7, 0.5, ptr(out_faces), H, None, None),
                 lambda: lib.smesh_segment_stats_despeckle_labels(seg._h, ptr(measure), H, 0.5, None, H, None, None),
                 lambda: lib.smesh_segment_stats_despeckle_rows(seg._h, ptr(measure), H, 0.5, ptr(rows), H, 0, ptr(rows), H),
                 lambda: lib.smesh_segment_stats_despeckle_rows(seg._h, ptr(measure), H, 0.5, None, H, 5, ptr(rows), H),
                 lambda: lib.smesh_aggregator_segment_stats_despeckle(None, seg._h, ptr(measure), H, 0.5, ptr(rows), H),
                 lambda: lib.smesh_segment_stats_face_areas(None, ptr(faces), ptr(vertices), H, ptr(w), H),
                 lambda: lib.smesh_segment_stats_face_areas(graph._h, ptr(faces), ptr(vertices), 7, ptr(w), H),
                 lambda: lib.smesh_segment_stats_face_areas(graph._h, ptr(faces), None, H, ptr(w), H)):
        with pytest.raises(ValueError):
            _lib.check(call())
    bad_faces = faces.copy()
    bad_faces[11, 2] = V                                           # an index outside [0, V) is found on the device
    with pytest.raises(ValueError):
        _lib.check(lib.smesh_segment_stats_face_areas(graph._h, ptr(bad_faces), ptr(vertices), H, ptr(w), H))
    # every out pointer of members() may be NULL; labels alone are an output
    _lib.check(lib.smesh_segment_stats_members(seg._h, None, None, H))
    _lib.check(lib.smesh_segment_stats_pool(seg._h, ptr(rows), H, 5, None, H, SUMS, 0.9, None, ptr(out_labels), H))
    assert (out_labels == -1).all()                                # all-zero rows: don't care
