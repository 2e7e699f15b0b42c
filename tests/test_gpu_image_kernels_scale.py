"""The image-side kernels past the sizes at which their launches change, against the numpy restatements (tests/probs_labels_ref.py,
tests/depth_gate_ref.py, tests/view_weights_ref.py, tests/edge_gate_ref.py, tests/label_prep_ref.py, tests/label_colors_ref.py,
tests/resize_ref.py) on the cases of tests/image_kernels_scale_cases.py.  The sibling modules stop at images of 130 x 67 (class
vectors), 200 x 180 (weights planes) and 300 x 150 (label images); the workload's are 1296 x 968 and 1920 x 1080.  What only an image
of this size executes:

  A. the steady state of k_probs_labels_tiled -- the prefetch of the next tile, the carry of its pixel coordinates and ground truth,
     the final round that reloads its own tile, workgroups with different numbers of rounds -- and the grid-stride loop of
     k_probs_labels_generic: more tiles (rounds) than the capped grid has workgroups.  Every call asserts from the launch's own report
     ("last_probs_labels_grid" / "last_probs_labels_work") that work > 2 grid + grid / 4;
  B. the placement of k_depth_weights' and k_view_weights' chunks on the XCDs in runs, which is the identity up to 32 768 pixels:
     planes of 9 and 18 chunks, alone and inside a group beside views of 2 chunks;
  C. k_edge_weights in a group whose views have unlike tile grids, 2 x 3 and 4 x 1 in a launch of 4 x 3: the early return and the
     decoding of blockIdx.x by the launch's rows;
  D. the 64-bit branch of src_index (k_labels_prepare, k_labels_prepare_colors, k_depth_weights): sides over 32 768;
  E. the second turn of the resize kernels' column loop: an image 65 536 wide.

Every result here is defined to the bit, so every comparison is exact (floats as their uint32 patterns) and every expected value is
computed on the host.  The one exception is the fused result of B and C where a view queues triangles whose rows several lanes add
to: there the comparison is the project's assert_fused_close, as in the sibling tests (`same` of tests/test_gpu_view_weights.py); the
scenes are tessellated so finely that no view does, and the tests assert that, so the bit form is the one that runs.

Durations on an MI355X (`pytest --durations`, one run, each image and reference made by the first test that needs it): the whole
module, 40 tests, 6.5 s; the slowest test 1.1 s (40 classes in float16: 516 000 rows narrowed and arg-maxed on the host); the three
255-class images 0.3 - 1.0 s each, a counting case with a new image 0.4 - 0.7 s, everything else 0.1 s or less.
"""
import ctypes

import numpy as np
import pytest

import depth_gate_ref as dg
import edge_gate_ref as eg
import half_helpers as hh
import image_kernels_scale_cases as cases
import test_gpu_depth_gate as tdg
import test_gpu_probs_labels as tpl
import test_gpu_view_weights as tvw
import view_weights_ref as vw
from helpers import random_probs
from test_gpu_label_prep import bits, layouts, option

pytestmark = pytest.mark.gpu

C = 19
_cache = {}


def first_difference(got, want):
    """For a failure's message: the first element at which two arrays differ."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s and %s" % (got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(-1))
    if not len(bad):
        return "equal"
    k = np.unravel_index(int(bad[0]), got.shape)
    return "%d of %d differ, first at %s: got %r, want %r" % (len(bad), got.size, k, got[k], want[k])


def assert_equal(got, want, what):
    assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))


# ---- A. the probs-labels loops ---------------------------------------------------------------------------------------------------
def assert_three_rounds(sm, name, layout, counting):
    """The last launch shared out what the case was sized for, over few enough workgroups that each took two tiles (rounds) and at
    least a quarter of them a third."""
    grid, work = option(sm, "last_probs_labels_grid"), option(sm, "last_probs_labels_work")
    path, planned = cases.pl_work(name, layout)
    print("    %s, %s: %s path, work %d over a grid of %d" % (name, layout, path, work, grid))
    assert work == planned, "%s, %s: the launch reports %d units of work, the %s path gives this shape %d" % (name, layout, work, path, planned)
    assert 0 < grid and work > 2 * grid + grid // 4, (
        "%s, %s: a grid of %d workgroups for %d units of work is fewer than three rounds with a partial third (the shape is computed "
        "for %d CUs and a cap of %d workgroups)" % (name, layout, grid, work, cases.CUS, cases.pl_cap(counting)))


LABEL_CASES = [(name, layout) for name, case in cases.PL_CASES.items() if not case[4] for layout in case[3]]
COUNT_CASES = [(name, layout, gdt) for name, case in cases.PL_CASES.items() if case[4] for layout in case[3] for gdt in cases.COUNT_GT_DTYPES]


@pytest.mark.parametrize("name,layout", LABEL_CASES, ids=[("%s-%s" % c).replace(" ", "_") for c in LABEL_CASES])
def test_labels_over_three_rounds_per_workgroup(sm, name, layout):
    classes, dtype, shape, _, _ = cases.PL_CASES[name]
    assert option(sm, "probs_labels_tiles") == 1
    vals, wide, want = cases.pl_case_image(name)
    dev = tpl.device_layout(vals, layout)
    for thr in cases.THRESHOLDS:
        lab, dc = want[thr]
        assert len(np.unique(lab)) > 1 and (thr is None or 0.15 < dc.mean() < 0.6)
        got = sm.fusion.argmax_labels_device(dev, dont_care_threshold=thr, **tpl.kw(dtype))
        assert_three_rounds(sm, name, layout, False)
        assert got.shape == shape and got.dtype == np.uint8
        assert_equal(got.numpy(), tpl.expected_image(lab, dc, 255, np.uint8), "%s, %s, threshold %s" % (name, layout, thr))


@pytest.mark.parametrize("name,layout,gt_dtype", COUNT_CASES, ids=[("%s-%s-%s" % c).replace(" ", "_") for c in COUNT_CASES])
def test_counting_over_three_rounds_per_workgroup(sm, name, layout, gt_dtype):
    """The matrix against np.add.at and the label image of the same pass, with both values of confusion_wave_aggregate."""
    from semantic_meshes_amd.device import to_device
    classes, dtype, shape, _, _ = cases.PL_CASES[name]
    vals, wide, want = cases.pl_case_image(name)
    dev = tpl.device_layout(vals, layout)
    gt = to_device(cases.pl_ground_truth(classes, shape, gt_dtype))
    cm = sm.fusion.ConfusionMatrix(classes)
    before = option(sm, "confusion_wave_aggregate")
    try:
        for aggregate in (0, 1):
            sm._lib.set_option("confusion_wave_aggregate", aggregate)
            for thr in cases.THRESHOLDS:
                lab, dc = want[thr]
                M, ignored = cases.pl_matrix(name, gt_dtype, thr)
                assert ignored > 0 and (thr is None or M[:, classes].sum() > 0)
                cm.reset()
                out = cm.add_probs(dev, gt, dont_care_threshold=thr, labels_out=True, **tpl.kw(dtype))
                assert_three_rounds(sm, name, layout, True)
                what = "%s, %s, %s, threshold %s, aggregate %d" % (name, layout, gt_dtype, thr, aggregate)
                assert_equal(cm.get(), M, "matrix of " + what)
                assert cm.ignored == ignored, what
                assert_equal(out.numpy(), tpl.expected_image(lab, dc, 255, np.uint8), "labels of " + what)
    finally:
        sm._lib.set_option("confusion_wave_aggregate", before)


# ---- B. depth and view weights in runs per XCD -----------------------------------------------------------------------------------
def offset_plane(plane):
    """`plane` on the device four bytes behind a 16-byte boundary: the kernels' one-by-one form."""
    from semantic_meshes_amd.device import DeviceArray, to_device
    flat = to_device(np.concatenate([np.zeros(1, np.float32), plane.reshape(-1)]))
    off = DeviceArray(flat.ptr + 4, plane.shape, np.float32, flat.device, owner=flat)
    assert off.ptr % 16 == 4
    return off


def poison(shape):
    """A float32 plane of NaN made on the device and dropped again.  The Python layer allocates a call's weights plane itself, and a
    block just freed is what the next allocation of its size gets: without this a chunk that a kernel skips shows the previous call's
    weights, which are the expected ones (seen when a deliberately broken k_depth_weights left 18 of 71 033 pixels different).  Best
    effort -- the counts, which are exact, notice a skipped chunk whatever the allocator does."""
    from semantic_meshes_amd.device import to_device
    plane = to_device(np.full(shape, np.nan, np.float32))
    del plane


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("size", cases.PLANES, ids=lambda s: "%dx%d" % s)
def test_depth_weights_of_a_plane_dealt_in_runs(sm, size, dtype):
    """uint16 and float32 sensors, dense and as the transposed view of an (h,w) image, with and without a weights-in plane: the bits
    of depth_gate_ref.weights and its counts, one launch a call; at the larger size also from an unaligned depth plane."""
    from semantic_meshes_amd.device import to_device
    assert cases.per_xcd(size) >= 2
    depth = tdg.rendered_depth(sm, size)
    rng = np.random.default_rng([size[0], size[1], 7 if dtype == np.float32 else 0])
    sensor = tdg.make_sensor(rng, depth, cases.SENSOR_SHAPES[size], dtype)
    w_in = rng.uniform(0.1, 2.0, size=size).astype(np.float32)
    gate, g = sm.fusion.DepthGate(0.05, 0.004, None, 6.5, "drop"), dg.gate(0.05, 0.004, None, 6.5, "drop", dtype)
    d_depth, d_w = to_device(depth), to_device(w_in)
    images = layouts(sensor, True)
    for weights in (None, w_in):
        want, want_counts = dg.weights(depth, sensor, g, weights)
        assert (want_counts > 0).all() and (want != 0).any()
        for layout in ("dense", "transposed"):
            poison(size)
            before = option(sm, "depth_weights_launches")
            got, counts = sm.fusion.depth_weights(d_depth, images[layout], gate, None if weights is None else d_w, return_counts=True)
            assert option(sm, "depth_weights_launches") - before == 1
            what = "%s %s sensor, weights-in %s" % (layout, np.dtype(dtype).name, weights is not None)
            assert_equal(bits(got), bits(want), "weights, " + what)
            assert_equal(counts, want_counts, "counts, " + what)
    if size == cases.PLANES[0]:
        want, want_counts = dg.weights(depth, sensor, g, w_in)
        off = offset_plane(depth)
        poison(size)
        got, counts = sm.fusion.depth_weights(off, images["dense"], gate, d_w, return_counts=True)
        assert_equal(bits(got), bits(want), "weights from an unaligned depth plane")
        assert_equal(counts, want_counts, "counts from an unaligned depth plane")


@pytest.mark.parametrize("size", cases.PLANES, ids=lambda s: "%dx%d" % s)
def test_view_weights_of_a_plane_dealt_in_runs(sm, size):
    """Every spec of tests/test_gpu_view_weights.py, with and without a weights-in plane: the bits of view_weights_ref.weights and
    its counts; at the larger size also with an unaligned weights-in plane."""
    from semantic_meshes_amd.device import to_device
    assert cases.per_xcd(size) >= 2
    mesh, cam, r, idx, depth, normals, w_in = tvw.check_kernel_against_restatement(sm, size)
    if size == cases.PLANES[0]:
        args = (4, 0.3, False, 6.5, 3.0)
        want, want_counts = vw.weights(cam, normals, idx, depth, vw.spec(*args), w_in)
        got, counts = sm.fusion.view_weights(r, cam, to_device(idx), to_device(depth), sm.fusion.ViewWeights(*args), offset_plane(w_in), return_counts=True)
        assert_equal(bits(got), bits(want), "weights from an unaligned weights-in plane")
        assert_equal(counts, want_counts, "counts from an unaligned weights-in plane")


def scene(sm, key, grid, sizes, rewind):
    """Nine ring cameras over synth.grid_mesh(*grid), alternating between the two resolutions, with the render's own planes, class
    vectors, the caller's weights and uint16 sensor images of one size, a third of whose samples are off; built once and left
    unchanged.  `rewind`: every third face looks away from the cameras (the rasteriser does not cull), for the view weights."""
    if key not in _cache:
        from semantic_meshes_amd import synth
        from semantic_meshes_amd.data import Mesh
        mesh = synth.grid_mesh(*grid)
        if rewind:
            faces = np.array(mesh.faces, np.int32)
            faces[::3] = faces[::3, ::-1]
            mesh = Mesh(np.asarray(mesh.vertices, np.float32), faces)
        cams = [synth.ring_camera(k, cases.GROUP_VIEWS, *sizes[k % 2]) for k in range(cases.GROUP_VIEWS)]
        r = sm.render.triangles(mesh)
        rng = np.random.default_rng([grid[0], sizes[0][0], sizes[1][0]])
        idx, depth, probs, mine, sensors, queued = [], [], [], [], [], 0
        sw, sh = cases.GROUP_SENSOR
        for cam in cams:
            i, d = (np.array(p) for p in r.render(cam))
            queued += int(r.render_stats(cam, queues=True)[1][0])
            assert i.shape == d.shape == tuple(cam.resolution) and np.isfinite(d).any()
            idx.append(i)
            depth.append(d)
            probs.append(np.maximum(random_probs(rng, *cam.resolution, C), 1e-3).astype(np.float32))
            mine.append(rng.uniform(0.1, 2.0, size=cam.resolution).astype(np.float32))
            near = d[dg.axis_index(d.shape[0], sw)[:, None], dg.axis_index(d.shape[1], sh)[None, :]].astype(np.float64)
            mm = np.where(np.isfinite(near), np.rint(1000.0 * near + np.where(rng.random(near.shape) < 0.3, 500.0, 0.0)), 0.0)
            sensors.append(mm.astype(np.uint16))
        for a in idx + depth + probs + mine + sensors:
            a.setflags(write=False)
        print("    %s: %d faces, %d queued triangles over the nine views" % (key, len(mesh.faces), queued))
        _cache[key] = dict(mesh=mesh, cams=cams, idx=idx, depth=depth, probs=probs, mine=mine, sensors=sensors, P=len(mesh.faces),
                           normals=vw.face_normals(mesh.vertices, mesh.faces), exact=queued == 0)
    return _cache[key]


def group_scene(sm):
    """(283, 251) and (96, 64) inside one group, over a grid of 102 400 faces: no triangle box over 8 x 8 pixels at either size."""
    return scene(sm, "group", (320, 160), cases.GROUP_SIZES, True)


def twin(sm, sc, planes, weighted, counter):
    """The plain call with the restatement's planes and the weighted call: the same kernel, `counter` advanced by two (a group of
    eight and one more view), the fused rows equal -- in bits, since no view of these scenes queues a triangle."""
    from semantic_meshes_amd.device import to_device
    r = sm.render.triangles(sc["mesh"])
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in planes])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C)
    before = option(sm, counter)
    stats = weighted(got, r, d_probs)
    assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith("k_fuse_tri")
    assert option(sm, counter) - before == 2
    assert sc["exact"]          # (no queued triangle: `same` compares bits)
    tvw.same(sc, "sum", got, plain)
    return stats


def test_depth_gated_group_with_a_large_and_a_small_view(sm):
    """fuse_views(sensor_depths=, depth_gate=, depth_stats=True): the grid of the launch is the large view's, 3 chunks per XCD; the
    small views' 2 chunks go to workgroups 0 and 8 of theirs."""
    from semantic_meshes_amd.device import to_device
    sc = group_scene(sm)
    g = dg.gate(0.02, missing="drop")
    ref = [dg.weights(sc["depth"][k], sc["sensors"][k], g, sc["mine"][k]) for k in range(cases.GROUP_VIEWS)]
    planes, counts = [w for w, _ in ref], np.stack([c for _, c in ref])
    assert (counts[:, dg.INCONSISTENT] > 0).all() and (counts[:, dg.VISIBLE] > counts[:, dg.INCONSISTENT]).all()
    stats = twin(sm, sc, planes, lambda a, r, d_probs: a.fuse_views(
        r, sc["cams"], d_probs, [to_device(w) for w in sc["mine"]], sensor_depths=[to_device(s) for s in sc["sensors"]],
        depth_gate=sm.fusion.DepthGate(0.02, missing="drop"), depth_stats=True), "depth_weights_launches")
    assert stats.shape == (cases.GROUP_VIEWS, 4) and stats.dtype == np.uint64
    assert_equal(stats, counts, "per-view counts")


def test_view_weighted_group_with_a_large_and_a_small_view(sm):
    """fuse_views(view_weights=, view_stats=True) over the same views."""
    from semantic_meshes_amd.device import to_device
    sc = group_scene(sm)
    s = vw.spec(*tvw.SPEC)
    ref = [vw.weights(sc["cams"][k], sc["normals"], sc["idx"][k], sc["depth"][k], s, sc["mine"][k]) for k in range(cases.GROUP_VIEWS)]
    planes, counts = [w for w, _ in ref], np.stack([c for _, c in ref])
    assert (counts[:, 1:] > 0).any(axis=0).all() and all(0 < (w > 0).sum() for w in planes)
    stats = twin(sm, sc, planes, lambda a, r, d_probs: a.fuse_views(
        r, sc["cams"], d_probs, [to_device(w) for w in sc["mine"]], view_weights=sm.fusion.ViewWeights(*tvw.SPEC), view_stats=True),
        "view_weights_launches")
    assert stats.shape == (cases.GROUP_VIEWS, 4) and stats.dtype == np.uint64
    assert_equal(stats, counts, "per-view counts")


# ---- C. the edge gate with unlike tile grids in one launch -----------------------------------------------------------------------
@pytest.mark.parametrize("gate_args", cases.EDGE_GATES, ids=lambda a: "radius%d" % a[0])
def test_edge_gated_group_whose_views_have_unlike_tile_grids(sm, gate_args):
    """fuse_views(edge_gate=, edge_stats=True) over nine views that alternate (40, 130) and (100, 30): a launch of 4 x 3 tiles, of
    which one view uses 2 x 3 and the other 4 x 1.  Against edge_gate_ref.weights, the brute-force form.
    (What this catches: a launch whose rows come from another view than the tallest, or whose columns from another than the widest,
    leaves tiles of one view unwritten -- tried with the rows of the widest view, both radii fail.  What it cannot catch, because it is
    no error: a kernel that decodes blockIdx.x by the VIEW's own rows also visits every tile of the view once, with other workgroups.)"""
    from semantic_meshes_amd.device import to_device
    sc = scene(sm, "edge", (160, 80), cases.EDGE_SIZES, False)
    g = eg.gate(*gate_args)
    ref = [eg.weights(sc["depth"][k], g, sc["mine"][k]) for k in range(cases.GROUP_VIEWS)]
    planes, counts = [w for w, _ in ref], np.stack([c for _, c in ref])
    print("    counts per view\n%s" % counts)
    assert (counts[:, 1:].sum(axis=1) > 0).all() and all(0 < (w > 0).sum() for w in planes)
    stats = twin(sm, sc, planes, lambda a, r, d_probs: a.fuse_views(
        r, sc["cams"], d_probs, [to_device(w) for w in sc["mine"]], edge_gate=sm.fusion.EdgeGate(*gate_args), edge_stats=True),
        "edge_weights_launches")
    assert stats.shape == (cases.GROUP_VIEWS, 4) and stats.dtype == np.uint64
    assert_equal(stats, counts, "per-view counts")


# ---- D. sides over 32 768 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", cases.LONG_AXES, ids=["x", "y"])
def test_label_images_sampled_over_a_side_of_65536(sm, axis):
    """prepare_labels(resize="nearest") with and without a map, and with a palette, from 40 000 to 65 536 pixels along one axis: the
    planes of label_prep_ref / label_colors_ref, whose index arithmetic is int64."""
    from semantic_meshes_amd.device import to_device
    size = cases.long_shape(cases.LONG_TARGET, axis)
    for classes in cases.LONG_CLASSES:
        for with_map in (False, True):
            src, m, want = cases.long_labels(axis, classes, with_map)
            for where, image in (("host", src), ("device", to_device(src))):
                before = option(sm, "labels_prepare_launches")
                out = sm.fusion.prepare_labels(image, classes, size, "nearest", m)
                assert option(sm, "labels_prepare_launches") - before == 1
                assert out.dtype == want.dtype
                assert_equal(out, want, "%d classes, map %s, %s image" % (classes, with_map, where))
        img, colors, cls, want = cases.long_colors(axis, classes)
        before = option(sm, "labels_colors_launches")
        out = sm.fusion.prepare_labels(to_device(img), classes, size, "nearest", palette=sm.fusion.ColorTable(colors, cls))
        assert option(sm, "labels_colors_launches") - before == 1
        assert_equal(out, want, "%d classes, palette" % classes)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("axis", cases.LONG_AXES, ids=["x", "y"])
def test_depth_weights_sampled_over_a_side_of_65536(sm, axis, dtype):
    from semantic_meshes_amd.device import to_device
    depth, sensor, w_in, (want, want_counts) = cases.long_depth(axis, dtype)
    d_depth, d_sensor, d_w = to_device(depth), to_device(sensor), to_device(w_in)
    poison(depth.shape)
    got, counts = sm.fusion.depth_weights(d_depth, d_sensor, sm.fusion.DepthGate(*cases.LONG_GATE), d_w, return_counts=True)
    assert_equal(bits(got), bits(want), "weights")
    assert_equal(counts, want_counts, "counts")


# ---- E. width 65 536 through the resize kernels ----------------------------------------------------------------------------------
def probs_code(L, dtype):
    return {"float32": L.PROBS_F32, "float16": L.PROBS_F16, "bfloat16": L.PROBS_BF16}[dtype]


@pytest.mark.parametrize("classes,dtype", [(8, "float32"), (8, "float16"), (5, "float32")], ids=["vector-float32", "vector-float16", "generic"])
def test_resize_probs_to_a_width_of_65536(sm, classes, dtype):
    """smesh_resize_probs into an output filled with -7, which no result holds: 8 classes take the vector path, 5 the generic one.
    Column 65 535 is the second turn of the loop of the workgroups with blockIdx.y == 0."""
    from semantic_meshes_amd.device import to_device
    L, lib = sm._lib, sm._lib.lib()
    (w, h), (W, H) = cases.WIDE_SOURCE, cases.WIDE_TARGET
    values, wide = cases.wide_source(classes, dtype)
    want = hh.narrow(cases.wide_resized(classes, dtype), dtype) if dtype != "float32" else cases.wide_resized(classes, dtype)
    src = to_device(values)
    out = to_device(np.full((W, H, classes), -7.0, np.float32 if dtype == "float32" else np.float16))
    code = probs_code(L, dtype)
    L.check(lib.smesh_resize_probs(ctypes.c_void_p(src.ptr), code, None, L.MEM_DEVICE, w, h, classes, ctypes.c_void_p(out.ptr), code, W, H, L.RESIZE_BILINEAR, 0))
    L.synchronize(0)
    got = np.asarray(out) if dtype == "float32" else np.asarray(out).view(np.uint16)
    assert_equal(got[W - 1], want[W - 1], "the last column")
    assert_equal(got, want, "the image")


@pytest.mark.parametrize("vector", [1, 0], ids=["vector", "generic"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_labels_of_an_image_resampled_to_a_width_of_65536(sm, dtype, vector):
    """smesh_resize_probs_labels, VEC on and off, into a label image filled with 200, which is no label and no don't-care code."""
    from semantic_meshes_amd.device import to_device
    L, lib = sm._lib, sm._lib.lib()
    (w, h), (W, H) = cases.WIDE_SOURCE, cases.WIDE_TARGET
    classes = cases.WIDE_LABEL_CLASSES
    values, wide = cases.wide_label_source(dtype)
    src = to_device(values)
    before = option(sm, "resize_vector")
    sm._lib.set_option("resize_vector", vector)
    try:
        for thr in cases.THRESHOLDS:
            lab, dc = cases.wide_labels(dtype, thr)
            want = np.where(dc, 255, lab).astype(np.uint8)
            canvas = to_device(np.full((W, H), 200, np.uint8))
            L.check(lib.smesh_resize_probs_labels(ctypes.c_void_p(src.ptr), probs_code(L, dtype), None, L.MEM_DEVICE, w, h, classes,
                                                  float("-inf") if thr is None else thr, ctypes.c_void_p(canvas.ptr), L.LBL_CODES["uint8"], None, 255,
                                                  W, H, L.RESIZE_BILINEAR, 0))
            L.synchronize(0)
            got = np.asarray(canvas)
            assert_equal(got[W - 1], want[W - 1], "the last column, threshold %s" % thr)
            assert_equal(got, want, "the label image, threshold %s" % thr)
    finally:
        sm._lib.set_option("resize_vector", before)
