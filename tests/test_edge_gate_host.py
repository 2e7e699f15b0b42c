"""Fusion gated at occlusion edges (include/smesh_edge_gate.h), without a GPU: the header against the ctypes table, the POD layout,
`EdgeGate`'s validation, the keyword errors that must come before the library is touched, and the brute-force restatement against a
second, separable numpy form on random planes -- checked with edge_gate_ref and numpy alone."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import edge_gate_ref as eg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smesh_edge_gate.h")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_is_c99_and_agrees_with_the_ctypes_table():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.EDGE_GATE_SIGNATURES) == ["smesh_edge_weights", "smesh_fuse_views_weighted"]
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.EDGE_GATE_SIGNATURES[name][1]), name
    others = set()
    for table in dir(_lib):
        if table.endswith("SIGNATURES") and table != "EDGE_GATE_SIGNATURES":
            others |= set(getattr(_lib, table))
    assert not set(declared) & others

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert define("SMESH_EDGE_MAX_RADIUS") == _lib.EDGE_MAX_RADIUS == eg.MAX_RADIUS == 8
    assert (define("SMESH_EDGE_TILE_X"), define("SMESH_EDGE_TILE_Y")) == (_lib.EDGE_TILE_X, _lib.EDGE_TILE_Y)
    # the weighted call is the view-weights call plus the edge gate and its counts
    assert len(_lib.EDGE_GATE_SIGNATURES["smesh_fuse_views_weighted"][1]) == len(_lib.VIEW_WEIGHTS_SIGNATURES["smesh_fuse_views_view_weights"][1]) + 2
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(declared) <= names


def test_the_pod_has_the_headers_layout():
    from semantic_meshes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fields = re.search(r"typedef struct smesh_edge_gate \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.EdgeGatePOD._fields_] == ["radius", "abs_tol", "rel_tol", "behind", "front", "silhouette"]
    assert re.findall(r"(\w+)\s+\w+;", fields) == ["int32_t", "float", "float", "int32_t", "int32_t", "int32_t"]
    assert ctypes.sizeof(_lib.EdgeGatePOD) == 24
    assert [getattr(_lib.EdgeGatePOD, f).offset for f, _ in _lib.EdgeGatePOD._fields_] == [0, 4, 8, 12, 16, 20]


def test_edge_gate_checks_its_numbers():
    from semantic_meshes_amd.fusion import EdgeGate
    g = EdgeGate(3, 0.05)
    assert (g.radius, g.abs_tol, g.rel_tol, g.behind, g.front, g.silhouette) == (3, float(np.float32(0.05)), 0.0, True, False, False)
    pod = EdgeGate(8, 0.25, 0.5, False, True, True)._pod()
    assert (pod.radius, pod.abs_tol, pod.rel_tol, pod.behind, pod.front, pod.silhouette) == (8, 0.25, 0.5, 0, 1, 1)
    same = eg.gate(8, 0.25, 0.5, False, True, True)
    assert (pod.radius, np.float32(pod.abs_tol), np.float32(pod.rel_tol), bool(pod.behind), bool(pod.front), bool(pod.silhouette)) == tuple(same)
    assert repr(EdgeGate(2, 0.5, 0.25, True, True, False)) == "EdgeGate(radius=2, abs_tol=0.5, rel_tol=0.25, behind=True, front=True, silhouette=False)"
    with pytest.raises(TypeError):
        EdgeGate(3)                                  # abs_tol has no default
    for args, kw in (((0, 0.1), {}), ((9, 0.1), {}), ((-1, 0.1), {}), ((1.5, 0.1), {}), (("2", 0.1), {}), ((True, 0.1), {}), ((None, 0.1), {}),
                     ((2, np.nan), {}), ((2, -0.1), {}), ((2, np.inf), {}), ((2, "x"), {}), ((2, None), {}),
                     ((2, 0.1), dict(rel_tol=np.nan)), ((2, 0.1), dict(rel_tol=-1.0)), ((2, 0.1), dict(rel_tol="x")),
                     ((2, 0.1), dict(behind=1)), ((2, 0.1), dict(front=None)), ((2, 0.1), dict(silhouette=0)), ((2, 0.1), dict(behind="yes"))):
        with pytest.raises(ValueError):
            EdgeGate(*args, **kw)
    assert EdgeGate(1, 0).radius == 1 and EdgeGate(np.int64(8), 0.0).radius == 8 and EdgeGate(2, 0.1, behind=np.bool_(False)).behind is False


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
    probs, mask = np.zeros((8, 6, 5), np.float32), np.zeros((8, 6), np.uint8)
    gate = fusion.EdgeGate(2, 0.1)
    calls = {"fuse_views": lambda **kw: a.fuse_views(r, [cam, cam], [probs, probs], **kw),
             "fuse_views_labels": lambda **kw: a.fuse_views_labels(r, [cam, cam], [mask, mask], **kw),
             "fuse_view": lambda **kw: a.fuse_view(r, cam, probs, **kw),
             "fuse_view_labels": lambda **kw: a.fuse_view_labels(r, cam, mask, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="edge_stats=True needs edge_gate"):
            call(edge_stats=True)
        with pytest.raises(ValueError, match="fusion.EdgeGate"):
            call(edge_gate=(2, 0.1))
        with pytest.raises(ValueError, match="depth_stats"):
            call(edge_gate=gate, depth_stats=True)             # a depth consumer without a depth gate
        with pytest.raises(ValueError, match="view_stats"):
            call(edge_gate=gate, view_stats=True)
        with pytest.raises(ValueError, match="go together"):
            call(edge_gate=gate, depth_gate=fusion.DepthGate(0.05))
        assert {"edge_gate", "edge_stats"} <= set(inspect.signature(getattr(fusion._MeshAggregator, name)).parameters), name
    for name in ("fuse_views", "fuse_view"):
        with pytest.raises(ValueError, match="sample_in_kernel"):
            calls[name](edge_gate=gate, resize="bilinear", sample_in_kernel=True)
    with pytest.raises(ValueError, match="fusion.EdgeGate"):
        fusion.edge_weights_device(np.zeros((8, 6), np.float32), 2)
    with pytest.raises(ValueError, match="rank 2"):
        fusion.edge_weights_device(np.zeros((8, 6, 1), np.float32), gate)
    # the entry points that do not take the keywords: their route is edge_weights_device + a weights image
    for name in ("fuse_views_ranged", "add", "add_many", "add_labels"):
        assert "edge_gate" not in inspect.signature(getattr(fusion._MeshAggregator, name)).parameters, name
    # the stats come back in the order (view, edge, depth), only those asked for, a single one bare
    got = [fusion._stats_of("view", "depth", v, d, edge_counts="edge", edge_stats=e) for v in (False, True) for e in (False, True) for d in (False, True)]
    assert got == [None, "depth", "edge", ("edge", "depth"), "view", ("view", "depth"), ("view", "edge"), ("view", "edge", "depth")]


@pytest.mark.parametrize("radius", [1, 2, 3, 8])
def test_the_restatement_against_the_separable_form(radius):
    """Random planes of two levels, NaN, -inf and +inf, images smaller than the window included: the brute-force window and the
    separable one agree in bits, weights and counts, under every combination of the flags."""
    rng = np.random.default_rng(radius)
    seen = np.zeros(4, np.uint64)
    for W, H in ((1, 1), (1, 9), (5, 3), (23, 31), (40, 17)):
        d = eg.random_plane(rng, W, H, background=0.06)
        pick = rng.random((W, H))
        d[pick < 0.01] = np.nan
        d[(pick > 0.01) & (pick < 0.02)] = -np.inf
        d = np.where(np.isfinite(d), d + rng.uniform(0, 0.2, (W, H)).astype(np.float32), d).astype(np.float32)
        w_in = rng.uniform(0.1, 2.0, (W, H)).astype(np.float32)
        for a, b in zip(eg.window(d, radius), eg.window_separable(d, radius)):
            np.testing.assert_array_equal(a, b)
        for flags in range(8):
            g = eg.gate(radius, 0.1, 0.02, bool(flags & 1), bool(flags & 2), bool(flags & 4))
            w, counts = eg.weights(d, g, w_in)
            w2, counts2 = eg.weights_separable(d, g, w_in)
            np.testing.assert_array_equal(bits(w), bits(w2))
            np.testing.assert_array_equal(counts, counts2)
            visible = np.isfinite(d)
            assert counts[eg.VISIBLE] == visible.sum() and not w[~visible].any()
            assert (w == 0)[visible].sum() == counts[1:].sum()         # w_in > 0: a kept pixel keeps a weight > 0
            if flags == 0:
                np.testing.assert_array_equal(bits(w), np.where(visible, bits(w_in), 0))
            seen += counts
    assert (seen > 0).all(), seen


def test_the_restatement_on_a_case_worked_by_hand():
    """A 7 x 1 column: far far NEAR far far bg far, radius 1."""
    d = np.array([[5, 5, 2, 5, 5, np.inf, 5]], np.float32)
    w, c = eg.weights(d, eg.gate(1, 0.5, behind=True, front=True, silhouette=True))
    #                 far  far(near in window) near(far in window) far(near) far(bg) bg far(bg)
    assert list(w[0]) == [1, 0, 0, 0, 0, 0, 0]
    assert list(c) == [6, 2, 1, 2]
    w, c = eg.weights(d, eg.gate(1, 0.5))
    assert list(w[0]) == [1, 0, 1, 0, 1, 0, 1] and list(c) == [6, 2, 0, 0]
    w, c = eg.weights(d, eg.gate(2, 3.0))            # the step of 3 is not above t = 3
    assert list(w[0]) == [1, 1, 1, 1, 1, 0, 1] and list(c) == [6, 0, 0, 0]
