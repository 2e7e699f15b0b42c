"""Label-image fusion on the GPU: MeshAggregator.add_labels / fuse_view_labels / fuse_views_labels (include/smesh_labels.h) against the
CPU oracle fed the one-hot of the same labels (tf.one_hot: a label outside [0, C) is the all-zero vector)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from helpers import assert_fused_close, small_scene
from test_gpu_fuzz import _room
from test_labels_host import one_hot

pytestmark = pytest.mark.gpu

NATIVE = "k_fuse_tri_labels"


def random_labels(rng, W, H, C, dtype=np.int32, bad=0.03):
    lab = rng.integers(0, C, size=(W, H)).astype(np.int64)
    out = rng.random((W, H)) < bad
    lab[out] = rng.choice([-1, C, C + 1], size=int(out.sum()))
    info = np.iinfo(dtype)
    return np.clip(lab, info.min, info.max).astype(dtype)


def lds_max_classes(sm):
    """Up to this class count k_fuse_tri_labels keeps a wave's rows in LDS; beyond, the owner lane read-modify-writes global memory."""
    import ctypes
    v = ctypes.c_int64()
    sm._lib.check(sm._lib.lib().smesh_get_option(b"labels_lds_max_classes", ctypes.byref(v)))
    return int(v.value)


def expected_launches(n, cap):
    """Fusion launches of n label views: raster groups of eight, in each the largest of 8 / 4 / 2 / 1 views that fits the rest and `cap`."""
    launches = 0
    for start in range(0, n, 8):
        left = min(8, n - start)
        while left:
            nv = 1
            while nv * 2 <= min(cap, left):
                nv *= 2
            left -= nv
            launches += 1
    return launches


def fuse_slot_counts(sm, call):
    """(fusion launches, views they fused) of `call`, from the profile slot of the fusion kernels."""
    import ctypes
    lib = sm._lib.lib()
    sm._lib.check(lib.smesh_profile_reset(0))
    sm._lib.check(lib.smesh_profile_enable(0, 1 << sm._lib.PROF_FUSE_SCATTER))
    try:
        call()
        sm._lib.synchronize(0)
        launches, views = ctypes.c_uint64(), ctypes.c_uint64()
        sm._lib.check(lib.smesh_profile_read_ex(0, sm._lib.PROF_FUSE_SCATTER, None, None, ctypes.byref(launches), ctypes.byref(views)))
    finally:
        sm._lib.check(lib.smesh_profile_enable(0, 0))
    return int(launches.value), int(views.value)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_cfg2_full_size_group_of_eight_bit_exact(sm, oracle):
    """bench.py's entry point with masks: eight cfg2 views, uint8 labels (about 3 % out of range) in device memory, one
    fuse_views_labels call.  Bit-equal to the float32 single-threaded oracle fed one_hot(labels)."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.device import to_device
    mesh, cams, C = synth.scene("cfg2")
    P = len(mesh.faces)
    views = [5, 31, 57, 83, 109, 135, 161, 187]
    W, H = cams[0].resolution
    rng = np.random.default_rng(2024)
    labels = []
    for _ in views:
        lab = rng.integers(0, C, size=(W, H), dtype=np.uint8)
        lab[rng.random((W, H)) < 0.03] = 255
        labels.append(lab)
    r = sm.render.triangles(mesh)
    agg = sm.fusion.MeshAggregator(P, C)
    agg.fuse_views_labels(r, [cams[k] for k in views], [to_device(lab) for lab in labels])
    assert sm._lib.last_fuse_kernel() == NATIVE
    got = agg.get_raw()
    for k in views:     # bit equality is a one-lane-per-row property: these views hold no queued (over 8 x 8) triangle
        r.render(cams[k])
        assert r.render_stats(cams[k], queues=True)[1][0] == 0
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    oagg = oracle.OracleAggregator(P, C)
    oracle.set_threads(8)
    try:
        oidx = [o.render(cams[k])[0] for k in views]
    finally:
        oracle.set_threads(1)
    for idx, lab in zip(oidx, labels):
        oagg.add(idx, one_hot(lab, C))
    want = oagg.get_raw()
    assert (np.abs(want).sum(axis=1) > 0).sum() > 900_000
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(agg.get()), bits(oagg.get()))


def _scene(sm, which, rng):
    from semantic_meshes_amd import synth
    if which == "small":
        mesh, cams = small_scene(views=8)
        return mesh, cams
    verts, faces, half = _room(rng, int(rng.choice([3, 8, 20])))
    W, H = 160, 120
    cams = []
    for _ in range(5):
        eye = rng.uniform(-0.85, 0.85, 3) * half
        target = rng.uniform(-1.0, 1.0, 3) * half
        R, t = synth.look_at(tuple(eye), tuple(target), up=(0, 0, 1))
        f = float(rng.uniform(0.35, 1.2)) * W
        cams.append(sm.data.Camera(R, t, np.array([W, H]), np.array([f, f]), np.array([W / 2.0, H / 2.0])))
    return types.SimpleNamespace(vertices=verts, faces=faces), cams


CASES = [(which, kind, C) for which in ("small", "room") for kind in ("sum", "summax", "mul") for C in (5, 19, 40, 150, 300)]


@pytest.mark.parametrize("which,kind,C", CASES)
def test_every_path_against_the_oracle_on_one_hot(sm, oracle, which, kind, C):
    from semantic_meshes_amd.device import to_device
    case = CASES.index((which, kind, C))
    rng = np.random.default_rng(500 + case)
    iew = [0.0, 0.5, 1.0][case % 3]
    with_weights = bool((case // 3) % 2)
    mesh, cams = _scene(sm, which, rng)
    P = len(mesh.faces)
    W, H = cams[0].resolution
    r = sm.render.triangles(mesh)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    agg = sm.fusion.MeshAggregator(P, C, kind, iew)
    oagg = oracle.OracleAggregator(P, C, kind, iew)
    # The float32 oracle adds a primitive's pixels one after the other: the reference for bit equality where one lane owns a row.  A
    # triangle over 8 x 8 pixels is summed by a wave (tree / atomic order); with hundreds of terms the float32 sequential sum itself
    # is off by more than 1e-5 of the exact sum, so there the reference is the oracle that accumulates in float64 (what the project's
    # room and soup tests compare their tree-ordered paths with), at the same default tolerance.
    oracle.set_accum_double(True)
    try:
        oagg64 = oracle.OracleAggregator(P, C, kind, iew)
    finally:
        oracle.set_accum_double(False)
    labels = [random_labels(rng, W, H, C) for _ in cams]
    weights = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) for _ in cams] if with_weights else None
    d_labels, d_weights = [to_device(lab) for lab in labels], None if weights is None else [to_device(w) for w in weights]
    launches, fused = fuse_slot_counts(sm, lambda: agg.fuse_views_labels(r, cams, d_labels, d_weights))
    kernel = sm._lib.last_fuse_kernel()
    assert (kernel == NATIVE) == (kind != "mul"), kernel
    if kind != "mul":
        # the views per launch are what SMESH_FUSE_VIEWS allows (the child runs of test_every_path_with_fewer_views_per_launch rely on it)
        cap = max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8")))
        print("    %d launches for %d views, at most %d per launch" % (launches, fused, cap))
        assert fused == len(cams) and launches == expected_launches(len(cams), cap), (launches, fused, cap)
        # A check of the CONSTANT only, not an observation of the launch: the dispatch is one comparison of the class count with
        # this limit (rows in LDS up to 255 classes: 5 .. 150 here; read-modify-write in global memory beyond: 300), and both forms
        # report the one kernel name.  That both forms compute the right sums is what the C = 150 and C = 300 cases show.
        assert lds_max_classes(sm) == 255 and (C <= 255) == (C != 300)
    queued = 0
    for k, cam in enumerate(cams):
        oidx = o.render(cam)[0]
        np.testing.assert_array_equal(np.asarray(r.render(cam)[0]), oidx)
        queued += int(r.render_stats(cam, queues=True)[1][0])
        oagg.add(oidx, one_hot(labels[k], C), None if weights is None else weights[k])
        oracle.set_accum_double(True)
        try:
            oagg64.add(oidx, one_hot(labels[k], C), None if weights is None else weights[k])
        finally:
            oracle.set_accum_double(False)
    got, want = agg.get_raw(), oagg.get_raw()
    print("%s %s C=%d iew=%g weights=%s queued=%d kernel=%s max|raw diff|=%g" % (which, kind, C, iew, with_weights, queued, kernel,
                                                                             np.nanmax(np.abs(got.astype(np.float64) - want))))
    if kind == "mul":
        # degenerate on one-hot input (log 0 = -inf for every class but one): the same as the class-vector call of the product
        ref = sm.fusion.MeshAggregator(P, C, kind, iew)
        ref.fuse_views(r, cams, [to_device(one_hot(lab, C)) for lab in labels], None if weights is None else [to_device(w) for w in weights])
        np.testing.assert_array_equal(bits(agg.get()), bits(ref.get()))
        return
    if queued == 0:
        np.testing.assert_array_equal(bits(got), bits(want))
        assert_fused_close(agg.get(), oagg.get())
    oracle.set_accum_double(True)
    try:
        want64, dist64 = oagg64.get_raw(), oagg64.get()
    finally:
        oracle.set_accum_double(False)
    print("    against the float64-accumulating oracle: max|raw diff|=%g" % np.nanmax(np.abs(got.astype(np.float64) - want64)))
    assert_fused_close(got, want64)
    assert_fused_close(agg.get(), dist64)


@pytest.mark.parametrize("nv", [1, 2, 4])
def test_every_path_with_fewer_views_per_launch(nv):
    """SMESH_FUSE_VIEWS caps the views per fusion launch (read once per process): the same cases in a child process."""
    env = dict(os.environ, SMESH_FUSE_VIEWS=str(nv))
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                          "test_every_path_against and not mul and (19 or 300)", "-p", "no:cacheprovider"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def _fixture(sm, oracle, C=19, kind="sum", views=5, seed=7):
    rng = np.random.default_rng(seed)
    mesh, cams = small_scene(a=160, b=80, views=views)      # finely tessellated: every box at most 8 x 8, one lane owns each row
    W, H = cams[0].resolution
    labels = [random_labels(rng, W, H, C) for _ in cams]
    return mesh, cams, labels, rng


def _assert_all_small(r, cams):
    """Bit equality between differently grouped calls is a one-lane-per-row property (queued triangles are summed by float adds in
    no fixed order): the scene must hold no triangle over 8 x 8 pixels."""
    for cam in cams:
        r.render(cam)
        assert r.render_stats(cam, queues=True)[1][0] == 0


def test_equivalent_calls_give_the_same_bits(sm, oracle):
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, labels, rng = _fixture(sm, oracle, C)
    P = len(mesh.faces)
    W, H = cams[0].resolution
    r = sm.render.triangles(mesh)
    _assert_all_small(r, cams)

    def batch(images):
        a = sm.fusion.MeshAggregator(P, C)
        a.fuse_views_labels(r, cams, images)
        assert sm._lib.last_fuse_kernel() == NATIVE
        return bits(a.get_raw())

    want = batch([to_device(narrow) for narrow in [sm.fusion.narrow_labels(lab, C) for lab in labels]])
    assert want.any()
    for defer in (True, False):
        a = sm.fusion.MeshAggregator(P, C)
        a.defer = defer
        for cam, lab in zip(cams, labels):
            a.add_labels(r.render(cam)[0], to_device(sm.fusion.narrow_labels(lab, C)))
        assert sm._lib.last_fuse_kernel() == NATIVE
        np.testing.assert_array_equal(bits(a.get_raw()), want)
    np.testing.assert_array_equal(batch([to_device(lab.astype(np.int64)) for lab in labels]), want)
    np.testing.assert_array_equal(batch([to_device(lab.astype(np.int32)) for lab in labels]), want)                 # with negatives
    np.testing.assert_array_equal(batch([to_device(sm.fusion.narrow_labels(lab, 1000)) for lab in labels]), want)  # uint16 planes
    np.testing.assert_array_equal(batch([to_device(np.ascontiguousarray(lab.T)).T for lab in labels]), want)       # (H,W) seen as (W,H)
    np.testing.assert_array_equal(batch([np.ascontiguousarray(lab.T).T for lab in labels]), want)                   # the same on the host
    np.testing.assert_array_equal(batch(labels), want)                                                              # host against device
    a = sm.fusion.MeshAggregator(P, C)
    for cam, lab in zip(cams, labels):
        a.fuse_view_labels(r, cam, lab)
    np.testing.assert_array_equal(bits(a.get_raw()), want)
    # the C entry point on a HOST image that is neither narrow nor dense (the Python layer narrows with numpy first and never gets
    # there): int32 with negatives, an (H,W) array at the strides of its (W,H) view -- staged as it is, narrowed on the device
    import ctypes
    a = sm.fusion.MeshAggregator(P, C)
    for cam, lab in zip(cams, labels):
        hw = np.ascontiguousarray(lab.T.astype(np.int32))
        sm._lib.check(sm._lib.lib().smesh_fuse_view_labels(r._h, a._h, ctypes.byref(cam._pod), hw.ctypes.data_as(ctypes.c_void_p),
                                                           sm._lib.LBL_CODES["int32"], (ctypes.c_int64 * 2)(1, W), None, sm._lib.MEM_HOST))
    assert sm._lib.last_fuse_kernel() == NATIVE
    np.testing.assert_array_equal(bits(a.get_raw()), want)


def _one_hot_twin(sm, r, P, C, kind, cams, labels, foreign=False):
    from semantic_meshes_amd.device import to_device
    a, b = sm.fusion.MeshAggregator(P, C, kind), sm.fusion.MeshAggregator(P, C, kind)
    for cam, lab in zip(cams, labels):
        if foreign:
            idx = np.asarray(r.render(cam)[0]).copy()
            idx[3, 5] = 0 if idx[3, 5] != 0 else 1
            a.add_labels(idx, lab)
            kernel = sm._lib.last_fuse_kernel()          # (hands deferred views over first: the label call's own kernel)
            b.add(idx, one_hot(lab, C))
        else:
            a.add_labels(r.render(cam)[0], to_device(lab))
            kernel = sm._lib.last_fuse_kernel()
            b.add(r.render(cam)[0], to_device(one_hot(lab, C)))
    assert_fused_close(a.get_raw(), b.get_raw())
    ga, gb = a.get(), b.get()
    assert np.array_equal(np.isnan(ga), np.isnan(gb))
    assert_fused_close(np.nan_to_num(ga), np.nan_to_num(gb))
    return kernel


def test_fallbacks_equal_the_one_hot_call(sm, oracle):
    C = 19
    mesh, cams, labels, rng = _fixture(sm, oracle, C, views=3)
    P = len(mesh.faces)
    r = sm.render.triangles(mesh)
    assert _one_hot_twin(sm, r, P, C, "sum", cams, labels, foreign=True) != NATIVE          # a foreign index image
    assert _one_hot_twin(sm, r, P, C, "mul", cams, labels) != NATIVE                        # Mul
    rt = sm.render.texels(mesh, cams, 0.05)
    assert _one_hot_twin(sm, rt, rt.getPrimitivesNum(), C, "sum", cams, labels) != NATIVE   # a texel renderer
    a, b = sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C), sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C)
    from semantic_meshes_amd.device import to_device
    a.fuse_views_labels(rt, cams, [to_device(lab) for lab in labels])
    b.fuse_views(rt, cams, [to_device(one_hot(lab, C)) for lab in labels])
    assert_fused_close(a.get_raw(), b.get_raw())


def test_reordered_mesh_falls_back_child():
    if os.environ.get("SMESH_REORDER") != "1":
        env = dict(os.environ, SMESH_REORDER="1")
        res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                              "test_reordered_mesh_falls_back_child", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
        return
    import semantic_meshes_amd as sm
    C = 19
    mesh, cams, labels, rng = _fixture(sm, None, C, views=3)
    r = sm.render.triangles(mesh)
    kernel = _one_hot_twin(sm, r, len(mesh.faces), C, "sum", cams, labels)
    assert kernel != NATIVE, "SMESH_REORDER=1 did not re-order this mesh, or the label kernel took a re-ordered mesh"


def test_errors_leave_the_aggregator_unchanged(sm, oracle):
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, labels, rng = _fixture(sm, oracle, C, views=2)
    P = len(mesh.faces)
    W, H = cams[0].resolution
    r = sm.render.triangles(mesh)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view_labels(r, cams[0], to_device(labels[0]))
    before = bits(a.get_raw()).copy()
    assert before.any()
    bad = [labels[1].astype(np.float32), labels[1][:, :-1], np.stack([labels[1]] * 2, axis=-1)]
    for lab in bad:
        with pytest.raises(ValueError):
            a.add_labels(r.render(cams[1])[0], lab)
        with pytest.raises(ValueError):
            a.fuse_view_labels(r, cams[1], lab)
        with pytest.raises(ValueError):
            a.fuse_views_labels(r, [cams[1]], [lab])
        with pytest.raises(ValueError):
            a.add_labels(np.asarray(r.render(cams[1])[0]), to_device(lab))
    np.testing.assert_array_equal(bits(a.get_raw()), before)


def test_label_views_and_probability_views_alternate(sm, oracle):
    from helpers import random_probs
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, labels, rng = _fixture(sm, oracle, C, views=8, seed=11)
    P = len(mesh.faces)
    W, H = cams[0].resolution
    r = sm.render.triangles(mesh)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    a, oagg = sm.fusion.MeshAggregator(P, C), oracle.OracleAggregator(P, C)
    for k, cam in enumerate(cams):
        oidx = o.render(cam)[0]
        if k % 3 == 1:
            probs = random_probs(rng, W, H, C)
            a.add(r.render(cam)[0], to_device(probs))
            oagg.add(oidx, probs)
        else:
            a.add_labels(r.render(cam)[0], to_device(sm.fusion.narrow_labels(labels[k], C)))
            oagg.add(oidx, one_hot(labels[k], C))
    got = a.get_raw()
    _assert_all_small(r, cams)
    assert got.any()
    np.testing.assert_array_equal(bits(got), bits(oagg.get_raw()))
