"""The plumbing that the mesh-side results share (csrc/mesh_host.hpp, semantic_meshes_amd/mesh_results.py) on the GPU, at the smallest
shapes where it can go wrong: every form of a `source` and both forms of an output give the same bits, nothing and null are
handled, the owner check keeps its texts, and VertexTransfer refuses a device array of another GPU.  References are the numpy
restatements of the neighbouring test files, never the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import face_graph_ref as gref
import face_segments_ref as sref
import points_ref as pref
import test_gpu_vertices as tv

pytestmark = pytest.mark.gpu

CLASS_COUNTS = [1, 19, 65]      # a one-lane group, a 32-lane group, more than one wave-wide chunk
THRESHOLD = 0.9
MAX_DISTANCE = 1.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def host(a):
    return a if isinstance(a, np.ndarray) else a.numpy()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def grid():
    """(faces int32 [8,3], vertices float32 [9,3], five points: four next to faces, the last beyond MAX_DISTANCE)."""
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(2, 2)
    faces, vertices = np.ascontiguousarray(mesh.faces, np.int32), np.ascontiguousarray(mesh.vertices, np.float32)
    points = vertices[faces[[0, 3, 5, 6, 7]]].mean(axis=1).astype(np.float32)
    points[:, 2] += np.float32(0.25)
    points[4, 2] += np.float32(100.0)
    for a in (faces, vertices, points):
        a.setflags(write=False)
    return faces, vertices, points


def final_rows(sm, n, C, seed):
    """(aggregator, its final rows float32 [n,C]): a Sum aggregator after set_raw; a third of the rows all zero."""
    rng = np.random.default_rng(seed)
    raw = (rng.random((n, C), dtype=np.float32) ** 3 + np.float32(1e-3)).astype(np.float32)
    raw[rng.random(n) < 1 / 3] = 0.0
    raw[0] = 1.0                                      # (row 0 is annotated whatever the draw)
    agg = sm.fusion.MeshAggregator(n, C, "sum")
    agg.set_raw(raw)
    rows = np.array(agg.get(), np.float32)
    rows.setflags(write=False)
    return agg, rows


def sources(rows, agg):
    """The four forms of a source that hold `rows`."""
    from semantic_meshes_amd.device import to_device
    wide = np.full((rows.shape[0], 2 * rows.shape[1]), np.float32(7.0), np.float32)
    wide[:, ::2] = rows
    view = wide[:, ::2]
    assert rows.shape[1] == 1 or not view.flags["C_CONTIGUOUS"]
    return {"array": np.array(rows), "view": view, "device": to_device(rows), "aggregator": agg}


def assert_all_equal(call, forms, want=None):
    """`call(source, on_device)` gives the same bits for every source and both output forms (and `want`, when given)."""
    first = None
    for name, source in forms.items():
        for on_device in (False, True):
            got = call(source, on_device)
            if got is None:                              # (the call has no device form)
                continue
            got = host(got)
            if first is None:
                first = got
                if want is not None:
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert np.array_equal(bits(got), bits(want)), "the %s source differs from the numpy restatement" % name
            assert got.dtype == first.dtype and got.shape == first.shape
            assert np.array_equal(bits(got), bits(first)), "source %s, on_device=%s differs" % (name, on_device)
    return first


# ---- 1. sources and outputs agree in bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_vertex_and_point_transfer_agree_over_sources_and_outputs(sm, C):
    faces, vertices, points = grid()
    F, V = len(faces), len(vertices)
    agg, rows = final_rows(sm, F, C, 10 + C)
    forms = sources(rows, agg)
    vt = sm.fusion.VertexTransfer(faces, V)
    sums = tv.np_sums(faces, V, rows)
    assert_all_equal(lambda s, dev: None if dev else vt.sums(s), forms, sums)
    ann = assert_all_equal(lambda s, dev: vt.annotations_device(s, THRESHOLD) if dev else vt.annotations(s, THRESHOLD), forms)
    tv.assert_annotations(ann, sums, THRESHOLD, C)
    assert_all_equal(lambda s, dev: vt.labels_device(s, THRESHOLD) if dev else vt.labels(s, THRESHOLD), forms, tv.np_labels(sums, THRESHOLD))

    index = sm.fusion.SurfaceIndex(vertices, faces)
    pt = sm.fusion.PointTransfer(index, points, MAX_DISTANCE)
    near, _ = pref.nearest(vertices, faces, points, MAX_DISTANCE)
    assert np.array_equal(pt.faces.numpy(), near) and near[4] == -1 and (near[:4] >= 0).all()
    picked = np.where((near >= 0)[:, None], rows[np.maximum(near, 0)], np.float32(0.0)).astype(np.float32)
    assert_all_equal(lambda s, dev: pt.sums_device(s) if dev else pt.sums(s), forms, picked)
    ann = assert_all_equal(lambda s, dev: pt.annotations_device(s, THRESHOLD) if dev else pt.annotations(s, THRESHOLD), forms)
    assert not ann[4].any()
    want = tv.np_labels(picked, THRESHOLD)
    want[near < 0] = -1
    assert_all_equal(lambda s, dev: pt.labels_device(s, THRESHOLD) if dev else pt.labels(s, THRESHOLD), forms, want)


@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_face_graph_and_segments_agree_over_sources_and_outputs(sm, C):
    faces, vertices, _ = grid()
    F, V = len(faces), len(vertices)
    agg, rows = final_rows(sm, F, C, 20 + C)
    forms = sources(rows, agg)
    graph = sm.fusion.FaceGraph(faces, V)
    offsets, nbr = gref.adjacency(faces, V)
    x, _ = gref.propagate(offsets, nbr, rows, 2, gref.SMOOTH, alpha=0.5)
    assert_all_equal(lambda s, dev: graph.smooth_sums_device(s, iterations=2) if dev else graph.smooth_sums(s, iterations=2), forms, x)
    x, tot = gref.propagate(offsets, nbr, rows, 2, gref.FILL, observed_threshold=THRESHOLD)
    assert_all_equal(lambda s, dev: graph.fill_labels_device(s, iterations=2) if dev else graph.fill_labels(s, iterations=2), forms,
                     gref.finish(x, tot, THRESHOLD)[0])

    labels = np.array([0, 0, 1, 0, 0, 2, 2, -1], np.int32)
    seg = graph.segments(labels)
    ids, _, _, size = sref.segments(offsets, nbr, labels)
    want = sref.despeckle_rows(rows, labels, ids, size, 2)
    assert_all_equal(lambda s, dev: seg.despeckle_sums_device(s, 2) if dev else seg.despeckle_sums(s, 2), forms, want)


@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_texel_face_annotations_agree_over_sources_and_outputs(sm, C):
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(2, 2)
    r = sm.render.texels(mesh, [synth.ring_camera(k, 3, 64, 48) for k in range(3)], 2.0)
    _, res, _ = r.texel_layout()
    P, F = r.getPrimitivesNum(), len(mesh.faces)
    agg, rows = final_rows(sm, P, C, 30 + C)
    n = res.astype(np.int64) * (res.astype(np.int64) + 1) // 2
    sums = np.zeros((F, C), np.float32)
    np.add.at(sums, np.repeat(np.arange(F), n), rows)            # ascending texel order, one float32 addition after another
    ann = assert_all_equal(lambda s, dev: r.face_annotations_device(s, THRESHOLD) if dev else r.face_annotations(s, THRESHOLD),
                           sources(rows, agg))
    tv.assert_annotations(ann, sums, THRESHOLD, C)


# ---- 2. nothing and null --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_an_empty_mesh_gives_results_of_the_right_shape(sm, on_device):
    """F = 0, V = 3: vertex results have three rows, point results one per point, face results none."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.device import to_device
    faces, vertices, C = np.zeros((0, 3), np.int32), np.zeros((3, 3), np.float32), 19
    points = np.zeros((5, 3), np.float32)
    vt, graph = sm.fusion.VertexTransfer(faces, 3), sm.fusion.FaceGraph(faces, 3)
    pt = sm.fusion.PointTransfer(sm.fusion.SurfaceIndex(vertices, faces), points, MAX_DISTANCE)
    seg = graph.segments(np.zeros(0, np.int32))
    assert (seg.num_faces, seg.count, graph.num_entries) == (0, 0, 0) and (pt.faces.numpy() == -1).all()
    r = sm.render.texels(sm.data.Mesh(vertices, faces), [synth.ring_camera(0, 1, 64, 48)], 2.0)
    assert r.getPrimitivesNum() == 0 and r.texel_layout()[0].shape == (0, 3)
    empty = np.zeros((0, C), np.float32)
    for source in (empty, to_device(empty)):
        for normalize in (True, False):              # (no texels, no faces: the gather of n = 0 rows)
            rows = host((r.face_annotations_device if on_device else r.face_annotations)(source, normalize=normalize))
            assert rows.shape == (0, C) and rows.dtype == np.float32
        if on_device:
            got = [vt.annotations_device(source), vt.labels_device(source), pt.sums_device(source), pt.annotations_device(source),
                   pt.labels_device(source), graph.smooth_sums_device(source, iterations=2), graph.fill_labels_device(source, iterations=2),
                   seg.despeckle_sums_device(source, 2)]
        else:
            assert vt.sums(source).shape == (3, C) and not vt.sums(source).any()
            got = [vt.annotations(source), vt.labels(source), pt.sums(source), pt.annotations(source), pt.labels(source),
                   graph.smooth_sums(source, iterations=2), graph.fill_labels(source, iterations=2), seg.despeckle_sums(source, 2)]
        got = [host(g) for g in got]
        assert [g.shape for g in got] == [(3, C), (3,), (5, C), (5, C), (5,), (0, C), (0,), (0, C)]
        assert [g.dtype for g in got] == [np.float32, np.int32, np.float32, np.float32, np.int32, np.float32, np.int32, np.float32]
        assert not got[0].any() and (got[1] == -1).all() and not got[2].any() and not got[3].any() and (got[4] == -1).all()


@pytest.mark.parametrize("on_device", [False, True])
def test_no_points_and_no_entries(sm, on_device):
    faces, vertices, _ = grid()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    near, dist2 = (index.nearest_device if on_device else index.nearest)(np.zeros((0, 3), np.float32))
    assert host(near).shape == (0,) and host(near).dtype == np.int32 and host(dist2).shape == (0,) and host(dist2).dtype == np.float32
    one = sm.fusion.FaceGraph(faces[:1], len(vertices))
    assert one.num_entries == 0
    w = host((one.normal_weights if on_device else one.normal_weights_host)(vertices))
    assert w.shape == (0,) and w.dtype == np.float32


def test_null_outputs_through_the_library(sm):
    from semantic_meshes_amd import _lib
    faces, vertices, points = grid()
    lib = _lib.lib()
    index = sm.fusion.SurfaceIndex(vertices, faces)
    want, _ = pref.nearest(vertices, faces, points, MAX_DISTANCE)
    out = np.full(len(points), -7, np.int32)
    _lib.check(lib.smesh_surface_index_nearest(index._h, ptr(points), len(points), _lib.MEM_HOST, MAX_DISTANCE, ptr(out), None, _lib.MEM_HOST))
    assert np.array_equal(out, want)
    graph = sm.fusion.FaceGraph(faces, len(vertices))
    labels = np.array([0, 0, 1, 0, 0, 2, 2, -1], np.int32)
    seg = graph.segments(labels)
    offsets, nbr = gref.adjacency(faces, len(vertices))
    for which, ref in enumerate(sref.segments(offsets, nbr, labels)):
        got = np.full(len(ref), 77, ref.dtype)
        args = [None] * 4
        args[which] = ptr(got)
        _lib.check(lib.smesh_face_segments_get(seg._h, *args, _lib.MEM_HOST))
        assert np.array_equal(got, ref)


# ---- 3. the owner check's texts -------------------------------------------------------------------------------------------------
def test_the_owner_check_keeps_its_texts(sm):
    from semantic_meshes_amd import _lib
    faces, vertices, _ = grid()
    F, V, C = len(faces), len(vertices), 5
    lib = _lib.lib()
    vt, graph = sm.fusion.VertexTransfer(faces, V), sm.fusion.FaceGraph(faces, V)
    seg = graph.segments(np.zeros(F, np.int32))
    agg = sm.fusion.MeshAggregator(F + 4, C)
    out, h = np.zeros((max(F, V) + 4, C), np.float32), ctypes.c_void_p()
    calls = [
        ("vertex annotations: the aggregator has %d primitives, the vertex map %d faces",
         lambda: lib.smesh_aggregator_vertex_annotations(agg._h, vt._h, _lib.VTX_SUMS, 0.9, ptr(out), None, _lib.MEM_HOST)),
        ("face propagate: the aggregator has %d primitives, the face graph %d faces",
         lambda: lib.smesh_aggregator_face_propagate(agg._h, graph._h, None, _lib.MEM_HOST, _lib.FG_SMOOTH, 1, 0.5, 0.9, _lib.VTX_SUMS, 0.9,
                                                     ptr(out), None, None, _lib.MEM_HOST)),
        ("face segments: the aggregator has %d primitives, the face graph %d faces",
         lambda: lib.smesh_aggregator_face_segments(agg._h, graph._h, 0.9, None, _lib.MEM_HOST, 0.0, ctypes.byref(h))),
        ("face segments: the aggregator has %d primitives, the segments %d faces",
         lambda: lib.smesh_aggregator_face_segments_despeckle(agg._h, seg._h, 2, ptr(out), _lib.MEM_HOST)),
    ]
    for text, call in calls:
        with pytest.raises(ValueError) as err:
            _lib.check(call())
        assert str(err.value) == text % (F + 4, F)
    assert not h.value


# ---- 4. VertexTransfer and the wrong device -------------------------------------------------------------------------------------
def test_vertex_transfer_refuses_rows_of_another_device(sm):
    from semantic_meshes_amd.device import DeviceArray, to_device
    faces, vertices, _ = grid()
    vt = sm.fusion.VertexTransfer(faces, len(vertices))
    real = to_device(np.zeros((len(faces), 5), np.float32))
    elsewhere = DeviceArray(real.ptr, real.shape, np.float32, vt.device + 1, owner=real)
    for call in (vt.sums, vt.annotations, vt.labels):
        with pytest.raises(ValueError, match="face rows lives on device"):
            call(elsewhere)
