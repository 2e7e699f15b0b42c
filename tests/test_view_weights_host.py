"""Fusion weighted by viewing geometry (include/smesh_view_weights.h), without a GPU: the numpy restatement against the analytic
float64 answer on a tilted quad, the identity spec, the order of the decisions and the partition of the counts, the header against the
ctypes table, `ViewWeights`' validation and the Python argument errors -- checked with view_weights_ref and numpy alone."""
import inspect
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import view_weights_ref as vw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smesh_view_weights.h")
W, H = 64, 48


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tilt", [0.0, 60.0, 80.0])
def test_the_restatement_against_the_analytic_cosine_on_a_tilted_quad(tilt):
    """One planar quad with normal +z, a camera whose axis is tilted by a known angle: c is the cosine of the angle between the
    normal and each pixel's ray (float64, from the world-space ray) to 1e-6, weight == c**power to 1e-5; at the principal point the
    angle is the tilt itself."""
    verts, faces = vw.quad_mesh()
    cam = vw.tilted_camera(tilt, W, H)
    idx, depth, d_world = vw.plane_render(cam)
    hit = idx != vw.BG
    assert hit.sum() > 200
    normals = vw.face_normals(verts, faces)
    np.testing.assert_array_equal(normals, np.array([[0, 0, 64], [0, 0, 64]], np.float32))      # e1 x e2 of an 8 x 8 quad, not normalised
    want = np.abs(d_world[..., 2]) / np.linalg.norm(d_world, axis=-1)
    c, dot, visible = vw.cosines(cam, normals, idx, depth)
    np.testing.assert_array_equal(visible, hit)
    assert np.abs(c.astype(np.float64) - want)[hit].max() <= 1e-6
    assert (dot[hit] < 0).all()                       # the quad faces the camera
    # the four central pixels lie half a pixel from the principal point: their rays are within atan(sqrt(0.5) / f) <= sqrt(0.5) / f
    # radians of the camera's axis, and |d cos / d angle| <= 1
    centre = want[W // 2 - 1:W // 2 + 1, H // 2 - 1:H // 2 + 1]
    assert np.abs(centre - math.cos(math.radians(tilt))).max() <= math.sqrt(0.5) / cam.focal_lengths[0]
    for power in (1, 2, 5):
        w, counts = vw.weights(cam, normals, idx, depth, vw.spec(power))
        assert np.abs(w.astype(np.float64) - want ** power)[hit].max() <= 1e-5
        assert not w[~hit].any()
        assert list(counts) == [hit.sum(), 0, 0, 0]
    # the cut-off angle, halfway between the two analytic cosines around the median: exactly the pixels below it (none within
    # 1e-6 of it: checked)
    if tilt != 0.0:
        ordered = np.sort(want[hit])
        gaps = np.diff(ordered)
        k = len(ordered) // 4 + int(np.argmax(gaps[len(ordered) // 4:3 * len(ordered) // 4]))
        cut = float(np.float32(0.5 * (ordered[k] + ordered[k + 1])))
        assert np.abs(want[hit] - cut).min() > 1e-6
        w, counts = vw.weights(cam, normals, idx, depth, vw.spec(1, min_cos=cut))
        np.testing.assert_array_equal(w == 0, ~hit | (want < np.float32(cut)))
        assert counts[vw.GRAZING] == (hit & (want < np.float32(cut))).sum() > 0


def scene(seed=0):
    """A view with every kind of pixel: the quad seen at 60 degrees, half of it re-wound to face away, one degenerate face, ids
    beyond the table, background, non-finite depths."""
    rng = np.random.default_rng(seed)
    verts, faces = vw.quad_mesh()
    faces = np.concatenate([faces, [[0, 2, 1]], [[0, 0, 1]]]).astype(np.int32)      # face 2 looks away, face 3 is degenerate
    cam = vw.tilted_camera(60.0, W, H)
    idx, depth, _ = vw.plane_render(cam)
    hit = idx != vw.BG
    pick = rng.random((W, H))
    idx = np.where(hit & (pick < 0.3), 2, idx).astype(np.uint32)
    idx = np.where(hit & (pick > 0.9), 3, idx).astype(np.uint32)
    idx = np.where(hit & (pick > 0.97), 4, idx).astype(np.uint32)                   # id >= F: background
    depth = np.where(hit & (pick > 0.6) & (pick < 0.62), np.float32(np.nan), depth).astype(np.float32)
    return cam, vw.face_normals(verts, faces), idx, depth, rng.uniform(0.1, 2.0, (W, H)).astype(np.float32)


def test_the_identity_spec_gives_w_in_in_bits():
    cam, normals, idx, depth, w_in = scene()
    w, counts = vw.weights(cam, normals, idx, depth, vw.spec(0), w_in)
    visible = np.isfinite(depth) & (idx != vw.BG) & (idx < len(normals))
    assert 0 < visible.sum() < W * H and (idx == 3).any() and (idx == 4).any()
    np.testing.assert_array_equal(bits(w), np.where(visible, bits(w_in), 0))
    assert list(counts) == [visible.sum(), 0, 0, 0]
    ones, _ = vw.weights(cam, normals, idx, depth, vw.spec(0))
    np.testing.assert_array_equal(ones, visible.astype(np.float32))


@pytest.mark.parametrize("s", [vw.spec(1), vw.spec(2, 0.3, False), vw.spec(4, 0.55, True, 7.0), vw.spec(1, 0.3, False, 7.0, 3.0), vw.spec(0, 0.0, False)],
                         ids=["cos", "one-sided", "far", "all", "backfacing-only"])
def test_the_counts_partition_the_visible_pixels(s):
    cam, normals, idx, depth, w_in = scene(1)
    w, counts = vw.weights(cam, normals, idx, depth, s, w_in)
    visible = np.isfinite(depth) & (idx != vw.BG) & (idx < len(normals))
    assert counts[vw.VISIBLE] == visible.sum()
    assert not w[~visible].any()
    # a kept pixel has a weight > 0 (w_in > 0, c > 0) -- but for the degenerate face, whose c = 0 passes a cut-off of 0
    zero_but_kept = visible & (idx == 3) & (s.min_cos == 0) & (s.power > 0) & ~(depth > s.max_depth)
    rejected = visible & (w == 0) & ~zero_but_kept
    assert rejected.sum() == counts[vw.FAR] + counts[vw.GRAZING] + counts[vw.BACKFACING]
    assert (w[visible & ~rejected & ~zero_but_kept] > 0).all()
    far = visible & (depth > s.max_depth)
    assert counts[vw.FAR] == far.sum()
    assert not w[far].any()
    if not s.two_sided:
        assert counts[vw.BACKFACING] == (visible & ~far & (idx == 2)).sum() > 0       # the re-wound face, and only it
    else:
        assert counts[vw.BACKFACING] == 0
    degenerate = visible & ~far & (idx == 3)
    assert degenerate.any()
    if s.min_cos > 0:
        assert not w[degenerate].any()            # a degenerate face is grazing under any cut-off
    if np.isfinite(s.max_depth):
        assert 0 < counts[vw.FAR] < counts[vw.VISIBLE]


def test_the_falloff_and_the_order_of_the_factors():
    cam, normals, idx, depth, w_in = scene(2)
    c, _, visible = vw.cosines(cam, normals, idx, depth)
    w, _ = vw.weights(cam, normals, idx, depth, vw.spec(2, falloff_depth=4.0), w_in)
    with np.errstate(invalid="ignore"):
        q = depth / np.float32(4.0)
        want = (w_in * ((np.float32(1) * c) * c)) * (np.float32(1) / (np.float32(1) + q * q))
    np.testing.assert_array_equal(bits(w)[visible], bits(want)[visible])
    assert (w[visible & (idx < 2)] < (w_in * c * c)[visible & (idx < 2)]).all()


def test_header_is_c99_and_agrees_with_the_ctypes_table():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.VIEW_WEIGHTS_SIGNATURES) == ["smesh_fuse_views_view_weights", "smesh_view_weights"]
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.VIEW_WEIGHTS_SIGNATURES[name][1]), name
    others = set()
    for table in dir(_lib):
        if table.endswith("SIGNATURES") and table != "VIEW_WEIGHTS_SIGNATURES":
            others |= set(getattr(_lib, table))
    assert not set(declared) & others
    assert int(re.search(r"#define\s+SMESH_VW_MAX_POWER\s+(\d+)", text).group(1)) == _lib.VW_MAX_POWER == vw.MAX_POWER
    fields = re.search(r"typedef struct smesh_view_weights_spec \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.ViewWeightsPOD._fields_]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(declared) <= names


def test_view_weights_checks_its_numbers():
    from semantic_meshes_amd.fusion import ViewWeights
    v = ViewWeights()
    assert (v.power, v.min_cos, v.two_sided, v.max_depth, v.falloff_depth) == (1, 0.0, True, None, None)
    pod = v._pod()
    assert (pod.power, pod.min_cos, pod.two_sided, pod.max_depth, pod.falloff_depth) == (1, 0.0, 1, np.inf, np.inf)
    pod = ViewWeights(4, 0.3, False, 9.0, 2.5)._pod()
    same = vw.spec(4, 0.3, False, 9.0, 2.5)
    assert (pod.power, np.float32(pod.min_cos), bool(pod.two_sided), np.float32(pod.max_depth), np.float32(pod.falloff_depth)) == tuple(same)
    assert repr(ViewWeights(2, 0.5, False, 9.0, 2.5)) == "ViewWeights(power=2, min_cos=0.5, two_sided=False, max_depth=9.0, falloff_depth=2.5)"
    for kw in (dict(power=-1), dict(power=17), dict(power=1.5), dict(power="2"), dict(power=True), dict(power=None), dict(min_cos=np.nan),
               dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos="x"), dict(two_sided=1), dict(two_sided=None), dict(max_depth=np.nan),
               dict(max_depth="far"), dict(falloff_depth=np.nan), dict(falloff_depth=0.0), dict(falloff_depth=-2.0), dict(falloff_depth="x")):
        with pytest.raises(ValueError):
            ViewWeights(**kw)
    assert ViewWeights(0).power == 0 and ViewWeights(16).power == 16 and ViewWeights(np.int32(3)).power == 3
    assert ViewWeights(min_cos=1.0).min_cos == 1.0 and ViewWeights(max_depth=np.inf).max_depth == np.inf
    assert ViewWeights(falloff_depth=np.inf)._pod().falloff_depth == np.inf


def _bare_aggregator(classes=5):
    """A MeshAggregator that never saw the library: argument errors must come before its handle is asked for."""
    from semantic_meshes_amd.fusion import _MeshAggregator
    a = object.__new__(_MeshAggregator)
    a.classes, a.device, a.defer, a._pending, a._handle = classes, 0, False, [], None
    return a


def test_keyword_errors_need_no_device():
    from semantic_meshes_amd import fusion
    a = _bare_aggregator()
    cam = types.SimpleNamespace(resolution=(8, 6), _pod=None)
    r = types.SimpleNamespace(device=0, _h=None)
    texel = types.SimpleNamespace(device=0, _h=None, is_texel=True)
    probs, mask = np.zeros((8, 6, 5), np.float32), np.zeros((8, 6), np.uint8)
    spec = fusion.ViewWeights(2, 0.3)
    calls = {"fuse_views": lambda rr=r, **kw: a.fuse_views(rr, [cam, cam], [probs, probs], **kw),
             "fuse_views_labels": lambda rr=r, **kw: a.fuse_views_labels(rr, [cam, cam], [mask, mask], **kw),
             "fuse_view": lambda rr=r, **kw: a.fuse_view(rr, cam, probs, **kw),
             "fuse_view_labels": lambda rr=r, **kw: a.fuse_view_labels(rr, cam, mask, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="view_stats=True needs view_weights"):
            call(view_stats=True)
        with pytest.raises(ValueError, match="fusion.ViewWeights"):
            call(view_weights=2)
        with pytest.raises(ValueError, match="triangle renderer"):
            call(rr=texel, view_weights=spec)
        with pytest.raises(ValueError, match="depth_stats"):
            call(view_weights=spec, depth_stats=True)          # a depth consumer without a depth gate
        with pytest.raises(ValueError, match="go together"):
            call(view_weights=spec, depth_gate=fusion.DepthGate(0.05))
        assert {"view_weights", "view_stats"} <= set(inspect.signature(getattr(fusion._MeshAggregator, name)).parameters), name
    for name in ("fuse_views", "fuse_view"):
        with pytest.raises(ValueError, match="sample_in_kernel"):
            calls[name](view_weights=spec, resize="bilinear", sample_in_kernel=True)
    with pytest.raises(ValueError, match="fusion.ViewWeights"):
        fusion.view_weights_device(r, cam, np.zeros((8, 6), np.uint32), np.zeros((8, 6), np.float32), 2)
    with pytest.raises(ValueError, match="triangle renderer"):
        fusion.view_weights_device(texel, cam, np.zeros((8, 6), np.uint32), np.zeros((8, 6), np.float32), spec)
    # the entry points that do not take the keywords: their route is view_weights_device + a weights image
    for name in ("fuse_views_ranged", "add", "add_many", "add_labels"):
        assert "view_weights" not in inspect.signature(getattr(fusion._MeshAggregator, name)).parameters, name
    assert _stats_shapes(fusion) == [None, "view", "depth", ("view", "depth")]


def _stats_shapes(fusion):
    """What the four combinations of view_stats / depth_stats return."""
    return [fusion._stats_of("view", "depth", v, d) for v, d in ((False, False), (True, False), (False, True), (True, True))]
