"""Fusion gated by sensor depth (include/smesh_depth.h), without a GPU: known answers of the numpy restatement at the tolerance's
edges, the missing-sample rules, the order of the decisions, the sampling against label_prep_ref, the header against the ctypes
table, the Python argument errors, and that the occluder scene of test_gpu_depth_gate.py gates a real share of every view --
checked with depth_gate_ref, numpy and the CPU oracle alone."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import depth_gate_ref as dg
import label_prep_ref as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smesh_depth.h")
INF = np.float32(np.inf)


def one(d_r, raw, g, w_in=None):
    """The weight and the counts of a single pixel."""
    w, c = dg.weights(np.array([[d_r]], np.float32), np.array([[raw]]), g, None if w_in is None else np.array([[w_in]], np.float32))
    return float(w[0, 0]), [int(x) for x in c]


KEPT, REJECTED = (1.0, [1, 0, 0, 0]), (0.0, [1, 0, 0, 1])


@pytest.mark.parametrize("g", [dg.gate(0.25, scale=1.0 / 1024), dg.gate(0.0, rel_tol=0.125, scale=1.0 / 1024)], ids=["abs", "rel"])
def test_known_answers_at_the_edges_of_the_tolerance(g):
    """scale = 1/1024 is exact in float32: raw 2048 is d_s = 2.0, and t = 0.25 either as abs_tol or as 0.125 * 2.0."""
    assert float(g.scale) * 1024 == 1.0
    raw = np.uint16(2048)
    up, down = np.nextafter(np.float32(2.25), INF), np.nextafter(np.float32(1.75), -INF)
    assert up > np.float32(2.25) and down < np.float32(1.75)
    assert one(2.25, raw, g) == KEPT            # diff == t
    assert one(up, raw, g) == REJECTED
    assert one(1.75, raw, g) == KEPT
    assert one(down, raw, g) == REJECTED
    assert one(2.0, raw, g, w_in=0.375) == (0.375, [1, 0, 0, 0])      # the caller's weight goes through


def test_missing_samples_under_both_policies():
    keep, drop = dg.gate(0.25, scale=1.0 / 1024), dg.gate(0.25, scale=1.0 / 1024, missing="drop")
    assert one(2.0, np.uint16(0), keep, w_in=0.5) == (0.5, [1, 0, 1, 0])
    assert one(2.0, np.uint16(0), drop, w_in=0.5) == (0.0, [1, 0, 1, 0])
    fkeep, fdrop = dg.gate(0.25, dtype=np.float32), dg.gate(0.25, missing="drop", dtype=np.float32)
    assert float(fkeep.scale) == 1.0 and dg.gate(0.25).scale == np.float32(0.001)      # the defaults of the two dtypes
    for raw in (np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf):
        assert one(2.0, np.float32(raw), fkeep) == (1.0, [1, 0, 1, 0]), raw
        assert one(2.0, np.float32(raw), fdrop) == (0.0, [1, 0, 1, 0]), raw
    assert one(2.0, np.float32(2.25), fkeep) == KEPT and one(2.0, np.float32(2.5), fkeep) == REJECTED


def test_background_and_the_order_of_the_decisions():
    g = dg.gate(0.25, scale=1.0 / 1024, max_depth=3.0)
    for raw in (np.uint16(0), np.uint16(2048)):
        assert one(np.inf, raw, g) == (0.0, [0, 0, 0, 0])            # background: weight 0, in no count
    assert one(3.0, np.uint16(3072), g) == KEPT                       # d_r == max_depth is not far
    far = np.nextafter(np.float32(3.0), INF)
    assert one(far, np.uint16(3072), g) == (0.0, [1, 1, 0, 0])
    assert one(far, np.uint16(0), g) == (0.0, [1, 1, 0, 0])           # far AND missing counts as far
    assert one(far, np.uint16(100), g) == (0.0, [1, 1, 0, 0])         # far AND inconsistent counts as far
    keep = dg.gate(0.25, scale=1.0 / 1024)
    assert one(2.0, np.uint16(0), keep)[1] == [1, 0, 1, 0]            # missing before inconsistent: d_s = 0 would be 2.0 off


@pytest.mark.parametrize("src,size", [((7, 5), (16, 12)), ((16, 12), (16, 12)), ((160, 120), (40, 30)), ((1, 1), (5, 3))])
def test_nearest_sampling_is_the_rule_of_the_label_images(src, size):
    rng = np.random.default_rng(src[0])
    for dtype in (np.uint16, np.float32):
        image = (rng.random(src) * 4000).astype(dtype)
        got = dg.sample(image, *size)
        assert got.dtype == dtype
        np.testing.assert_array_equal(got.astype(np.int64), lp.sample(image.astype(np.int64), *size))
        if src == size:
            np.testing.assert_array_equal(got, image)
    for k in (0, 1):
        np.testing.assert_array_equal(dg.axis_index(src[k], size[k]), lp.axis_index(src[k], size[k]))


def test_header_is_c99_and_agrees_with_the_ctypes_table():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.DEPTH_SIGNATURES) == ["smesh_depth_weights", "smesh_fuse_views_depth"]
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.DEPTH_SIGNATURES[name][1]), name
    others = set()
    for table in dir(_lib):
        if table.endswith("SIGNATURES") and table != "DEPTH_SIGNATURES":
            others |= set(getattr(_lib, table))
    assert not set(declared) & others
    codes = dict(re.findall(r"#define\s+(SMESH_DEPTH_\w+)\s+(\d+)", text))
    assert (int(codes["SMESH_DEPTH_U16"]), int(codes["SMESH_DEPTH_F32"])) == (_lib.DEPTH_U16, _lib.DEPTH_F32)
    assert [int(codes["SMESH_DEPTH_IMG_" + k]) for k in ("F32", "F16", "BF16")] == [_lib.PROBS_F32, _lib.PROBS_F16, _lib.PROBS_BF16]
    assert (int(codes["SMESH_DEPTH_IMG_LABELS_U8"]), int(codes["SMESH_DEPTH_IMG_LABELS_U16"])) == (_lib.DEPTH_IMG_LABELS_U8, _lib.DEPTH_IMG_LABELS_U16)
    fields = re.search(r"typedef struct smesh_depth_gate \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.DepthGatePOD._fields_]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(declared) <= names


def test_depth_gate_checks_its_numbers():
    from semantic_meshes_amd.fusion import DepthGate
    with pytest.raises(TypeError):
        DepthGate()                                   # abs_tol has no default
    g = DepthGate(0.05)
    assert (g.rel_tol, g.scale, g.max_depth, g.missing) == (0.0, None, None, "keep")
    assert g.scale_for(np.uint16) == 0.001 and g.scale_for(np.float32) == 1.0 and DepthGate(0.05, scale=0.5).scale_for(np.uint16) == 0.5
    pod = DepthGate(0.05, 0.01, None, 9.0, "drop")._pod(np.uint16)
    assert (np.float32(pod.scale), np.float32(pod.abs_tol), np.float32(pod.rel_tol), pod.max_depth, pod.missing_keep) == (
        np.float32(0.001), np.float32(0.05), np.float32(0.01), 9.0, 0)
    assert g._pod(np.float32).max_depth == np.inf and g._pod(np.float32).missing_keep == 1 and g._pod(np.float32).scale == 1.0
    same = dg.gate(0.05, 0.01, None, 9.0, "drop")
    assert (same.scale, same.abs_tol, same.rel_tol, same.max_depth) == tuple(np.float32(x) for x in (pod.scale, pod.abs_tol, pod.rel_tol, pod.max_depth))
    for kw in (dict(abs_tol=np.nan), dict(abs_tol=-0.1), dict(abs_tol="x"), dict(abs_tol=None), dict(abs_tol=np.inf),
               dict(abs_tol=0.1, rel_tol=np.nan), dict(abs_tol=0.1, rel_tol=-1.0), dict(abs_tol=0.1, scale=np.nan), dict(abs_tol=0.1, scale=-2.0),
               dict(abs_tol=0.1, max_depth=np.nan), dict(abs_tol=0.1, max_depth="far"), dict(abs_tol=0.1, missing="maybe"), dict(abs_tol=0.1, missing=True)):
        with pytest.raises(ValueError):
            DepthGate(**kw)
    assert DepthGate(0.1, max_depth=np.inf).max_depth == np.inf and DepthGate(0.1, max_depth=-1.0).max_depth == -1.0


def _bare_aggregator(classes=5):
    """A MeshAggregator that never saw the library: argument errors must come before its handle is asked for."""
    from semantic_meshes_amd.fusion import _MeshAggregator
    a = object.__new__(_MeshAggregator)
    a.classes, a.device, a.defer, a._pending, a._handle = classes, 0, False, [], None
    return a


def test_keyword_errors_need_no_device():
    from semantic_meshes_amd import fusion
    a = _bare_aggregator()
    W, H = 8, 6
    cam = types.SimpleNamespace(resolution=(W, H), _pod=None)
    r = types.SimpleNamespace(device=0, _h=None)
    probs, mask, sensor = np.zeros((W, H, 5), np.float32), np.zeros((W, H), np.uint8), np.zeros((W, H), np.uint16)
    g = fusion.DepthGate(0.05)
    many = {"fuse_views": lambda **kw: a.fuse_views(r, [cam, cam], [probs, probs], **kw),
            "fuse_views_labels": lambda **kw: a.fuse_views_labels(r, [cam, cam], [mask, mask], **kw)}
    single = {"fuse_view": lambda **kw: a.fuse_view(r, cam, probs, **kw), "fuse_view_labels": lambda **kw: a.fuse_view_labels(r, cam, mask, **kw)}
    for name, call in many.items():
        with pytest.raises(ValueError, match="go together"):
            call(sensor_depths=[sensor, sensor])
        with pytest.raises(ValueError, match="go together"):
            call(depth_gate=g)
        with pytest.raises(ValueError, match="one sensor depth image per camera"):
            call(sensor_depths=[sensor], depth_gate=g)
        with pytest.raises(ValueError, match="fusion.DepthGate"):
            call(sensor_depths=[sensor, sensor], depth_gate=0.05)
        with pytest.raises(ValueError, match="depth_stats"):
            call(depth_stats=True)
        with pytest.raises(ValueError, match="uint16 or float32"):
            call(sensor_depths=[sensor, sensor.astype(np.int32)], depth_gate=g)
        with pytest.raises(ValueError, match="empty"):
            call(sensor_depths=[sensor, np.zeros((0, 3), np.uint16)], depth_gate=g)
    for name, call in single.items():
        with pytest.raises(ValueError, match="go together"):
            call(sensor_depth=sensor)
        with pytest.raises(ValueError, match="go together"):
            call(depth_gate=g)
        with pytest.raises(ValueError, match="depth_stats"):
            call(depth_stats=True)
    for call in (lambda **kw: a.fuse_views(r, [cam], [probs], sensor_depths=[sensor], depth_gate=g, **kw),
                 lambda **kw: a.fuse_view(r, cam, probs, sensor_depth=sensor, depth_gate=g, **kw)):
        with pytest.raises(ValueError, match="sample_in_kernel"):
            call(resize="bilinear", sample_in_kernel=True)
    with pytest.raises(ValueError, match="fusion.DepthGate"):
        fusion.depth_weights_device(np.zeros((W, H), np.float32), sensor, 0.05)
    with pytest.raises(ValueError, match="uint16 or float32"):
        fusion.depth_weights_device(np.zeros((W, H), np.float32), sensor.astype(np.float64), g)
    with pytest.raises(ValueError, match="rank 2"):
        fusion.depth_weights_device(np.zeros(W, np.float32), sensor, g)
    # the entry points that do not take the keywords
    import inspect
    for name in ("fuse_views_ranged", "add", "add_many", "add_labels"):
        assert "depth_gate" not in inspect.signature(getattr(fusion._MeshAggregator, name)).parameters, name
    for name in ("fuse_view", "fuse_view_labels"):
        assert {"sensor_depth", "depth_gate", "depth_stats"} <= set(inspect.signature(getattr(fusion._MeshAggregator, name)).parameters), name
    for name in ("fuse_views", "fuse_views_labels"):
        assert {"sensor_depths", "depth_gate", "depth_stats"} <= set(inspect.signature(getattr(fusion._MeshAggregator, name)).parameters), name


@pytest.mark.parametrize("size", dg.OCCLUDER_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_occluder_scene_gates_a_real_share_of_every_view(oracle, size):
    """What test_gpu_depth_gate.py relies on, with the oracle's own depth planes: in each of the nine views the rejected pixels are
    exactly the pixels the quad covers, 17 % - 55 % of the visible ones; none is missing or far; no visible pixel lies within 1e-4
    of the tolerance's edge; with max_depth = 9 some view has far pixels and no view has only far pixels."""
    mesh, cams, oidx, odepth, sensors, covered = dg.occluder_scene(oracle, *size)
    g, g9 = dg.gate(0.02), dg.gate(0.02, max_depth=9.0)
    far_views = 0
    for k in range(dg.OCCLUDER_VIEWS):
        w, c = dg.weights(odepth[k], sensors[k], g)
        visible = np.isfinite(odepth[k])
        np.testing.assert_array_equal(visible, oidx[k] != np.uint32(0xFFFFFFFF))
        np.testing.assert_array_equal(visible & (w == 0), covered[k] & visible)
        assert c[dg.VISIBLE] == visible.sum() and c[dg.FAR] == 0 and c[dg.MISSING] == 0
        assert 0.17 <= c[dg.INCONSISTENT] / c[dg.VISIBLE] <= 0.55, (k, c)
        diff = np.abs(odepth[k] - sensors[k].astype(np.float32) * np.float32(0.001))[visible]
        assert np.abs(diff - np.float32(0.02)).min() > 1e-4
        c9 = dg.weights(odepth[k], sensors[k], g9)[1]
        assert c9[dg.FAR] < c9[dg.VISIBLE]
        far_views += int(c9[dg.FAR] > 0)
    assert far_views > 0
    assert max(float(d[np.isfinite(d)].max()) for d in odepth) > 10.0
