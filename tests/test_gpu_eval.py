"""Confusion matrices on the device (include/smesh_eval.h, semantic_meshes_amd/evaluation.py) and MeshAggregator.labels().

Every expected matrix is numpy (`np.add.at`) on inputs made here and on the ORACLE's index images; every expected label is the rule
of smesh_eval.h applied in numpy to the aggregator's own get().  Counts are integers: all comparisons are array_equal."""
import types

import numpy as np
import pytest

from helpers import BG, random_probs, small_scene

pytestmark = pytest.mark.gpu

LBL_DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64")


def _limit():
    from semantic_meshes_amd import evaluation
    return evaluation.lds_max_classes()


def expected_matrix(pred, gt, C):
    """(M uint64 [C, C + 1], ignored) of int predictions and ground truth of any shape; predictions outside [0, C) are don't care."""
    pred = np.asarray(pred).astype(np.int64).ravel()
    g = np.asarray(gt)
    g = (g.astype(np.int64) if g.dtype != np.uint64 else np.where(g < 2 ** 62, g, 2 ** 62).astype(np.int64)).ravel()
    ok = (g >= 0) & (g < C)
    p = np.where((pred >= 0) & (pred < C), pred, C)
    M = np.zeros((C, C + 1), np.uint64)
    np.add.at(M, (g[ok], p[ok]), 1)
    return M, int((~ok).sum())


def expected_image(idx, labels, gt, C):
    """expected_matrix for an index image: the prediction is labels[idx], don't care where idx is outside [0, P)."""
    idx = np.asarray(idx)
    P = len(labels)
    wide = idx.astype(np.int64) if idx.dtype != np.uint64 else np.where(idx < 2 ** 62, idx, 2 ** 62).astype(np.int64)
    valid = (wide >= 0) & (wide < P)
    pred = np.where(valid, np.asarray(labels, np.int64)[np.where(valid, wide, 0)] if P else -1, -1)
    return expected_matrix(pred, gt, C)


def make_gt(rng, shape, C, dtype):
    """Ground truth of `dtype`: classes in [0, C), about 3 % out of range (C, C + 7, the dtype's maximum; negative values for the
    signed dtypes).  Values the dtype cannot hold wrap -- the expectation is computed from the typed array."""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    g = rng.integers(0, C, size=shape).astype(np.int64)
    bad_values = [C, C + 7, min(int(info.max), 2 ** 62)] + ([-1, -C - 1, int(info.min)] if dt.kind == "i" else [])
    bad = rng.random(shape) < 0.03
    out = np.where(bad, rng.choice(np.array(bad_values, np.int64), size=shape), g).astype(dt)
    if dt == np.uint64:
        out[out == 2 ** 62] = info.max
    return out


def make_pred(rng, n, C):
    p = rng.integers(0, C, size=n).astype(np.int32)
    odd = rng.random(n) < 0.1
    p = np.where(odd, rng.choice(np.array([-1, C, C + 7], np.int32), size=n), p).astype(np.int32)
    if n >= 3:
        p[rng.permutation(n)[:3]] = [-1, C, C + 7]           # each of them at least once
    return p


def class_counts():
    L = _limit()
    return [1, 2, 19, 40, 41, L, L + 1]


@pytest.mark.parametrize("which", range(7))
def test_add_in_one_dimension(sm, which):
    from semantic_meshes_amd.device import to_device
    C = class_counts()[which]
    L = _limit()
    if C == L + 1 and (L + 1) * (L + 2) * 8 > 10 ** 9:
        pytest.skip("the matrix of %d classes would need more than 1 GB" % C)
    rng = np.random.default_rng(100 + which)
    cm = sm.fusion.ConfusionMatrix(C)
    sizes = (0, 1, 63, 5003) if C == L + 1 else (0, 1, 63, 100003)
    for n in sizes:
        pred = make_pred(rng, n, C)
        assert n < 3 or {-1, C, C + 7} <= set(pred.tolist())
        for dtype in LBL_DTYPES:
            gt = make_gt(rng, n, C, dtype)
            want, want_ignored = expected_matrix(pred, gt, C)
            if n >= 5003 and np.iinfo(gt.dtype).max >= C + 7:
                assert want_ignored > 0 and want[:, C].sum() > 0
            for on_device in (False, True):
                cm.reset()
                if on_device:
                    cm.add(to_device(pred), to_device(gt))
                else:
                    cm.add(pred, gt)
                assert np.array_equal(cm.get(), want), (C, n, dtype, on_device)
                assert cm.ignored == want_ignored, (C, n, dtype, on_device)


@pytest.fixture(params=[0, 1], ids=["plain", "aggregate"])
def wave_aggregate(request, sm):
    """Both forms of the counting kernel: every lane adds 1 for itself / lanes that share a key add their count once."""
    import ctypes
    lib = sm._lib.lib()
    before = ctypes.c_int64(0)
    sm._lib.check(lib.smesh_get_option(b"confusion_wave_aggregate", ctypes.byref(before)))
    sm._lib.check(lib.smesh_set_option(b"confusion_wave_aggregate", request.param))
    yield request.param
    sm._lib.check(lib.smesh_set_option(b"confusion_wave_aggregate", int(before.value)))


def test_both_forms_count_the_same(sm, wave_aggregate):
    """Random keys (every round of the aggregation and the lanes left over) in LDS and beyond it."""
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(21)
    for C in (3, 40, _limit() + 1):
        n = 20011
        pred, gt = make_pred(rng, n, C), make_gt(rng, n, C, "int16")
        runs = np.repeat(rng.integers(0, C, size=n // 97 + 1), 97)[:n]          # ... and long runs of one key, with a few strays
        gt2 = np.where(rng.random(n) < 0.02, gt, runs).astype(np.int16)
        cm = sm.fusion.ConfusionMatrix(C)
        for p, g in ((pred, gt), (runs.astype(np.int32), gt2)):
            want, want_ignored = expected_matrix(p, g, C)
            cm.reset()
            cm.add(to_device(p), to_device(g))
            assert np.array_equal(cm.get(), want) and cm.ignored == want_ignored, (C, wave_aggregate)


@pytest.mark.parametrize("beyond", [False, True])
def test_worst_contention(sm, beyond, wave_aggregate):
    """Every sample in ONE bin (the case the kernel's in-wave aggregation is for), then two alternating bins."""
    from semantic_meshes_amd.device import to_device
    C = _limit() + 1 if beyond else 40
    n = 2 ** 20 + 7
    cm = sm.fusion.ConfusionMatrix(C)
    g, p = C - 1, min(2, C - 1)
    cm.add(to_device(np.full(n, p, np.int32)), to_device(np.full(n, g, np.uint8 if C <= 255 else np.uint16)))
    M = cm.get()
    assert M[g, p] == n and M.sum() == n and cm.ignored == 0
    cm.reset()
    pred = np.where(np.arange(n) % 2 == 0, p, -1).astype(np.int32)           # bins (g, p) and (g, don't care)
    cm.add(to_device(pred), to_device(np.full(n, g, np.int32)))
    M = cm.get()
    assert M[g, p] == (n + 1) // 2 and M[g, C] == n // 2 and M.sum() == n and cm.ignored == 0


# ---- rendered views -------------------------------------------------------------------------------------------------------------
C_VIEW = 19


@pytest.fixture(scope="module")
def scenes(sm, oracle):
    """[(renderer, [camera ...], [oracle index image ...], P)]: the small scene at 160 x 120 (three views, with background) and a
    room seen from inside at 67 x 45 (clipped walls, no background).  Rendered once by the oracle; nothing here changes."""
    from semantic_meshes_amd import synth
    from test_gpu_fuzz import _room
    out = []
    mesh, cams = small_scene()
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    out.append((sm.render.triangles(mesh), cams, [o.render(c)[0] for c in cams], len(mesh.faces)))
    rng = np.random.default_rng(77)
    verts, faces, half = _room(rng, 8)
    W, H = 67, 45
    R, t = synth.look_at(tuple(0.3 * half), tuple(np.array([1.0, 0.4, -0.2]) * half), up=(0, 0, 1))
    cam = sm.data.Camera(R, t, np.array([W, H]), np.array([0.6 * W, 0.6 * W]), np.array([W / 2.0, H / 2.0]))
    o = oracle.OracleRenderer(verts, faces)
    out.append((sm.render.triangles(types.SimpleNamespace(vertices=verts, faces=faces)), [cam], [o.render(cam)[0]], len(faces)))
    for _, _, idxs, _ in out:
        for idx in idxs:
            idx.setflags(write=False)
    return out


def _label_table(rng, P, C):
    """int32 [P]: classes, -1 entries and a few labels beyond C."""
    return rng.integers(-1, C + 2, size=P).astype(np.int32)


def test_add_view(sm, scenes):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(5)
    C = C_VIEW
    cm = sm.fusion.ConfusionMatrix(C)
    saw_background = False
    for renderer, cams, idxs, P in scenes:
        labels = _label_table(rng, P, C)
        labels_dev = to_device(labels)
        for cam, oidx in zip(cams, idxs):
            W, H = cam.resolution
            saw_background = saw_background or bool((oidx == BG).any())
            for dtype in ("uint8", "int16", "int64"):
                gt = make_gt(rng, (W, H), C, dtype)
                want, want_ignored = expected_image(oidx, labels, gt, C)
                assert want[:, C].sum() > 0 and want_ignored > 0             # (don't-care predictions and ignored pixels are exercised)
                as_hw = np.ascontiguousarray(gt.T)                            # an (H,W) array, handed over as its transposed view
                for name, image in (("host dense", gt), ("host transposed", as_hw.T),
                                    ("device dense", to_device(gt)), ("device transposed", to_device(as_hw).T)):
                    cm.reset()
                    cm.add_view(renderer, cam, labels_dev if "device" in name else labels, image)
                    assert np.array_equal(cm.get(), want), (P, dtype, name)
                    assert cm.ignored == want_ignored, (P, dtype, name)
    assert saw_background


def test_add_views_in_groups_equals_numpy_and_single_views(sm, oracle):
    """Eleven views: a group of eight and a rest of three."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(6)
    C = 40
    mesh, _ = small_scene()
    cams = [synth.ring_camera(k, 11, 160, 120) for k in range(11)]
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    renderer = sm.render.triangles(mesh)
    P = len(mesh.faces)
    labels = _label_table(rng, P, C)
    gts = [make_gt(rng, (160, 120), C, "uint8") for _ in cams]
    want = np.zeros((C, C + 1), np.uint64)
    want_ignored = 0
    for cam, gt in zip(cams, gts):
        M, ign = expected_image(o.render(cam)[0], labels, gt, C)
        want += M
        want_ignored += ign
    assert want[:, C].sum() > 0
    labels_dev = to_device(labels)
    batch, single = sm.fusion.ConfusionMatrix(C), sm.fusion.ConfusionMatrix(C)
    batch.add_views(renderer, cams, labels_dev, [to_device(g) for g in gts])
    for cam, gt in zip(cams, gts):
        single.add_view(renderer, cam, labels_dev, gt)
    assert np.array_equal(batch.get(), want) and batch.ignored == want_ignored
    assert np.array_equal(single.get(), want) and single.ignored == want_ignored
    batch.reset()
    batch.add_views(renderer, cams, labels, gts)                              # host ground truth, host labels
    assert np.array_equal(batch.get(), want) and batch.ignored == want_ignored


@pytest.mark.parametrize("dtype", ["uint32", "int64"])
def test_add_image(sm, dtype):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(8)
    C, P, W, H = 41, 1000, 67, 45
    idx = rng.integers(0, P, size=(W, H)).astype(dtype)
    r = rng.random((W, H))
    idx[r < 0.1] = np.array(0xFFFFFFFF if dtype == "uint32" else -1).astype(dtype)      # background
    idx[(r >= 0.1) & (r < 0.15)] = P                                                    # indices beyond the table
    idx[(r >= 0.15) & (r < 0.2)] = P + 12345
    labels = _label_table(rng, P, C)
    gt = make_gt(rng, (W, H), C, "int16")
    want, want_ignored = expected_image(idx, labels, gt, C)
    assert want[:, C].sum() > W * H * 0.15
    cm = sm.fusion.ConfusionMatrix(C)
    idx_hw, gt_hw = np.ascontiguousarray(idx.T), np.ascontiguousarray(gt.T)
    for name, args in (("host", (idx, labels, gt)), ("device", (to_device(idx), to_device(labels), to_device(gt))),
                       ("host transposed", (idx_hw.T, labels, gt_hw.T)),
                       ("device transposed, host table", (to_device(idx_hw).T, labels, to_device(gt_hw).T))):
        cm.reset()
        cm.add_image(*args)
        assert np.array_equal(cm.get(), want), name
        assert cm.ignored == want_ignored, name


def test_texel_renderer(sm, oracle):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(9)
    C = C_VIEW
    mesh, cams = small_scene()
    renderer = sm.render.texels(mesh, cams, 0.5)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces, cams, 0.5)
    P = renderer.getPrimitivesNum()
    assert P == o.getPrimitivesNum() and P > len(mesh.faces)
    labels = _label_table(rng, P, C)                                           # one label per texel
    gt = make_gt(rng, cams[0].resolution, C, "uint8")
    oidx = o.render(cams[0])[0]
    assert oidx[oidx != BG].max() >= len(mesh.faces)                           # (texel indices, not face indices)
    want, want_ignored = expected_image(oidx, labels, gt, C)
    cm = sm.fusion.ConfusionMatrix(C)
    cm.add_view(renderer, cams[0], to_device(labels), gt)
    assert np.array_equal(cm.get(), want) and cm.ignored == want_ignored


# ---- aggregator.labels() ----------------------------------------------------------------------------------------------------------
def rule(rows, threshold):
    """The label rule of smesh_eval.h in numpy: float32, the row total in ascending class order."""
    rows = np.asarray(rows, np.float32)
    t = np.zeros(len(rows), np.float32)
    for c in range(rows.shape[1]):
        t = (t + rows[:, c]).astype(np.float32)
    lab = rows.argmax(axis=1).astype(np.int32)                                 # (the first of equal maxima: the lowest class)
    lab[t < np.float32(threshold)] = -1
    return lab


@pytest.mark.parametrize("kind", ["sum", "mul"])
@pytest.mark.parametrize("C", [5, 19, 150])
def test_aggregator_labels(sm, kind, C):
    from semantic_meshes_amd import synth
    rng = np.random.default_rng(11 * C)
    mesh = synth.grid_mesh(40, 20)
    W, H = 160, 120
    # three views from close by, which together leave part of the mesh unseen
    cams = [synth.ring_camera(k, 3, W, H, radius_scale=0.3) for k in range(3)]
    renderer = sm.render.triangles(mesh)
    P = len(mesh.faces)
    agg = sm.fusion.MeshAggregator(P, C, kind)
    for cam in cams:
        probs = random_probs(rng, W, H, C, zero_fraction=0.1)
        if kind == "mul":
            probs = np.where(probs.sum(-1, keepdims=True) > 0, np.maximum(probs, 1e-3), 0).astype(np.float32)
        # a constructed tie: in the left half of every image classes 1 and 3 share the largest value, bit for bit
        top = (probs.max(axis=-1) * 2).astype(np.float32)
        probs[: W // 2, :, 1] = np.where(probs[: W // 2].sum(-1) > 0, top[: W // 2], 0)
        probs[: W // 2, :, 3] = probs[: W // 2, :, 1]
        agg.fuse_view(renderer, cam, probs)
    rows = agg.get()
    assert not np.isnan(rows).any()
    best = rows.max(axis=1)
    tied = (rows[:, 1] == best) & (rows[:, 3] == best) & (best > 0)
    for threshold in (0.9, 0.0):
        want = rule(rows, threshold)
        got = agg.labels(threshold)
        assert got.dtype == np.int32 and got.shape == (P,)
        assert np.array_equal(got, want), (kind, C, threshold)
        dev = agg.labels_device(threshold)
        assert dev.dtype == np.int32 and dev.shape == (P,) and np.array_equal(dev.numpy(), got)
    if kind == "sum":
        untouched = (agg.get_raw() == 0).all(axis=1)
        assert untouched.any() and not untouched.all()
        assert (agg.labels(0.9)[untouched] == -1).all()
        assert tied.any() and (agg.labels(0.9)[tied] == 1).all()               # the lowest class among equals


# ---- accumulation, errors -----------------------------------------------------------------------------------------------------------
def test_accumulation_reset_and_add_counts(sm):
    rng = np.random.default_rng(12)
    C, n = 19, 4099
    p1, g1, p2, g2 = make_pred(rng, n, C), make_gt(rng, n, C, "uint8"), make_pred(rng, n, C), make_gt(rng, n, C, "int32")
    (M1, i1), (M2, i2) = expected_matrix(p1, g1, C), expected_matrix(p2, g2, C)
    cm = sm.fusion.ConfusionMatrix(C)
    assert not cm.get().any() and cm.ignored == 0
    cm.add(p1, g1)
    cm.add(p2, g2)
    assert np.array_equal(cm.get(), M1 + M2) and cm.ignored == i1 + i2
    assert cm.accuracy() == sm.fusion.confusion_accuracy(M1 + M2) and cm.mean_iou() == sm.fusion.confusion_mean_iou(M1 + M2)
    assert np.array_equal(cm.iou(), sm.fusion.confusion_iou(M1 + M2), equal_nan=True)
    cm.reset()
    assert not cm.get().any() and cm.ignored == 0
    cm.add(p1, g1)
    cm.add_counts(M2, i2)
    cm.add_counts(M2)
    assert np.array_equal(cm.get(), M1 + M2 + M2) and cm.ignored == i1 + i2
    with pytest.raises(ValueError):
        cm.add_counts(M2[:, :C])
    with pytest.raises(ValueError):
        cm.add_counts(M2.astype(np.float64))
    cm.reset()
    assert not cm.get().any() and cm.ignored == 0


def test_errors_leave_the_matrix_unchanged(sm, scenes):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(13)
    C = C_VIEW
    renderer, cams, idxs, P = scenes[0]
    cam, (W, H) = cams[0], cams[0].resolution
    labels, gt = _label_table(rng, P, C), make_gt(rng, (W, H), C, "uint8")
    cm = sm.fusion.ConfusionMatrix(C)
    cm.add_view(renderer, cam, labels, gt)
    before, ignored = cm.get(), cm.ignored
    assert before.any()
    idx = np.asarray(idxs[0])
    bad_calls = [
        lambda: cm.add_view(renderer, cam, labels[:-1], gt),                               # a wrong P
        lambda: cm.add_view(renderer, cam, to_device(np.append(labels, 0).astype(np.int32)), gt),
        lambda: cm.add_views(renderer, [cam, cam], labels[:-1], [gt, gt]),
        lambda: cm.add_view(renderer, cam, labels, gt[:, :-1]),                            # a wrong image shape
        lambda: cm.add_view(renderer, cam, labels, gt.T),
        lambda: cm.add_image(idx, labels, gt[:-1]),
        lambda: cm.add_view(renderer, cam, labels, gt.astype(np.float32)),                 # a float ground truth
        lambda: cm.add_image(idx, labels, to_device(gt.astype(np.float32))),
        lambda: cm.add(labels, gt.astype(np.float64).ravel()[:P]),
        lambda: cm.add_image(idx.astype(np.float32), labels, gt),
        lambda: cm.add(labels, gt.ravel()[:P - 1]),
        lambda: cm.add_views(renderer, [cam], labels, [gt, gt]),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert np.array_equal(cm.get(), before) and cm.ignored == ignored, k


def test_a_matrix_and_a_renderer_on_different_devices_are_refused(sm, scenes):
    from semantic_meshes_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("one device is visible")
    rng = np.random.default_rng(14)
    renderer, cams, _, P = scenes[0]
    cm = sm.fusion.ConfusionMatrix(C_VIEW, device=1)
    with pytest.raises(ValueError):
        cm.add_view(renderer, cams[0], _label_table(rng, P, C_VIEW), make_gt(rng, cams[0].resolution, C_VIEW, "uint8"))
    assert not cm.get().any() and cm.ignored == 0
