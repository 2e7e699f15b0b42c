"""Label images at their own resolution and in the dataset's ids (include/smesh_label_prep.h), without a GPU: the integer rule against
torch, the header against the ctypes table, the Python argument errors, and that the inputs of test_gpu_label_prep.py can show a
failure -- checked with label_prep_ref, numpy and the CPU oracle alone."""
import os
import re
import types

import numpy as np
import pytest

import label_prep_ref as lp
import resize_ref as ref
import sampled_inputs as si
from test_labels_host import one_hot
from test_sampled_host import fine_index_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXIS_PAIRS = sorted({(s[k], t[k]) for s, t in ref.SHAPES + lp.EXTRA_SHAPES for k in (0, 1)}
                    | {(480, 968), (640, 1296), (512, 1080), (1024, 1920)})


def test_the_integer_rule_is_nearest_exact():
    import torch
    for n, N in AXIS_PAIRS:
        src = torch.arange(n, dtype=torch.float32).view(1, 1, n)
        want = torch.nn.functional.interpolate(src, size=N, mode="nearest-exact").view(-1).numpy().astype(np.int64)
        got = lp.axis_index(n, N)
        np.testing.assert_array_equal(got, want, err_msg="%d -> %d" % (n, N))
        assert got.min() >= 0 and got.max() < n
    np.testing.assert_array_equal(lp.axis_index(7, 7), np.arange(7))


@pytest.mark.parametrize("n,N", [(5, 13), (37, 130)])
def test_the_legacy_rule_is_another_rule(n, N):
    """floor(X n / N) differs from the rule on at least one index: these sizes can tell the two apart."""
    assert (lp.axis_index(n, N) != lp.legacy_axis_index(n, N)).any()


def test_the_rule_needs_no_clamp_at_the_size_limits():
    for n, N in ((65536, 3), (65536, 65536), (1, 65536), (3, 65536)):
        i = lp.axis_index(n, N)
        assert i.min() >= 0 and i.max() < n and (np.diff(i) >= 0).all()
    assert (2 * 65535 + 1) * 65536 > 2 ** 32       # (just under 2^33: why the product is formed in 64 bits)


def test_header_and_ctypes_table_agree():
    from semantic_meshes_amd import _lib
    text = open(os.path.join(ROOT, "include", "smesh_label_prep.h")).read()
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.LABEL_PREP_SIGNATURES)
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.LABEL_PREP_SIGNATURES[name][1]), name
    assert int(re.search(r"#define SMESH_LABEL_PREP_MAP_LDS_MAX (\d+)", text).group(1)) == _lib.LABEL_PREP_MAP_LDS_MAX
    # each prepared entry point is its counterpart plus (w, h, map, map_len, map_memkind)
    for name in ("smesh_fuse_views_labels", "smesh_fuse_view_labels", "smesh_aggregator_add_labels"):
        assert _lib.LABEL_PREP_SIGNATURES[name + "_prepared"][1][:-5] == _lib.EXT_SIGNATURES[name][1]


def _bare_aggregator(classes=5):
    """A MeshAggregator that never saw the library: argument errors must come before its handle is asked for."""
    from semantic_meshes_amd.fusion import _MeshAggregator
    a = object.__new__(_MeshAggregator)
    a.classes, a.device, a.defer, a._pending, a._handle = classes, 0, False, [], None
    return a


def test_python_argument_errors_need_no_device():
    from semantic_meshes_amd import fusion
    from semantic_meshes_amd.evaluation import ConfusionMatrix
    a = _bare_aggregator()
    W, H = 8, 6
    idx = np.zeros((W, H), np.uint32)
    mask, small = np.zeros((W, H), np.uint8), np.zeros((4, 3), np.uint8)
    cam = types.SimpleNamespace(resolution=(W, H), _pod=None)
    r = types.SimpleNamespace(device=0, _h=None)
    calls = {"add_labels": lambda m, **kw: a.add_labels(idx, m, **kw),
             "fuse_view_labels": lambda m, **kw: a.fuse_view_labels(r, cam, m, **kw),
             "fuse_views_labels": lambda m, **kw: a.fuse_views_labels(r, [cam], [m], **kw),
             "prepare_labels_device": lambda m, **kw: fusion.prepare_labels_device(m, 5, (W, H), kw.get("resize"), kw.get("label_map"))}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="sampled, not blended"):
            call(small, resize="bilinear")
        with pytest.raises(ValueError, match="resize must be None"):
            call(small, resize=1)
        with pytest.raises(ValueError, match="one-dimensional"):
            call(mask, label_map=np.zeros((3, 3), np.int32))
        with pytest.raises(ValueError, match="integer table"):
            call(mask, label_map=np.zeros(3, np.float32))
        with pytest.raises(ValueError, match="empty"):
            call(mask, label_map=np.zeros(0, np.int32))
        with pytest.raises(ValueError, match="empty label image"):
            call(np.zeros((0, 3), np.uint8), resize="nearest")
        with pytest.raises(ValueError):      # a map does not excuse a size mismatch
            call(small, label_map=np.arange(4))
    # a size mismatch without the keyword: the messages of the plain calls, word for word
    with pytest.raises(ValueError, match=re.escape("Primitive image (8, 6), label image (4, 3) and weights image None must have the same width and height")):
        a.add_labels(idx, small)
    with pytest.raises(ValueError, match=re.escape("label image must be (W,H) = (8, 6), got (4, 3)")):
        a.fuse_view_labels(r, cam, small)
    with pytest.raises(ValueError, match=re.escape("label image 0 must be (W,H) = (8, 6), got (4, 3)")):
        a.fuse_views_labels(r, [cam], [small])
    with pytest.raises(ValueError, match="Primitive image"):
        a.add_labels(idx, small, label_map=np.arange(4))
    cm = object.__new__(ConfusionMatrix)
    cm.classes, cm.device, cm._h, cm._keep = 5, 0, None, []
    for kw in (dict(gt_resize="bilinear"), dict(gt_resize=1), dict(gt_map=np.zeros((2, 2), np.int32)), dict(gt_map=np.zeros(2, np.float32)),
               dict(gt_map=np.zeros(0, np.int64))):
        with pytest.raises(ValueError):
            cm._prepared_gt(mask, (W, H), kw.get("gt_resize"), kw.get("gt_map"), "ground truth")
    with pytest.raises(ValueError, match="must have shape"):
        cm._prepared_gt(small, (W, H), None, np.arange(4), "ground truth")
    assert cm._prepared_gt(mask, (W, H), "nearest", None, "ground truth") is mask      # nothing to prepare: the plain call


def test_the_class_vector_keyword_is_untouched():
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.resize import resize_mode
    assert _lib.RESIZE_MODES == {"bilinear": 1}
    with pytest.raises(ValueError):
        resize_mode("nearest")


def _masks(size, n, M):
    w, h = lp.FUSION_SOURCES[size]
    rng = np.random.default_rng(31 * w + h)
    return [lp.make_source(rng, w, h, np.int32, M) for _ in range(n)], lp.make_map(rng, M, 19)


@pytest.mark.parametrize("size", sorted(lp.FUSION_SOURCES))
def test_the_fusion_inputs_can_show_a_wrong_rule(oracle, size):
    """The oracle fed one_hot of (i) the correctly prepared masks against (ii) masks upsampled by the legacy rule, (iv) masks with the
    map skipped: different accumulator bits.  (iii) masks mapped BEFORE sampling: a map acts on each value by itself and nearest
    sampling only picks values, so map(sample(x)) == sample(map(x)) for every table, permutation or not -- the order stated in the
    header cannot be observed, and the test says so by asserting equal bits.  "half" is an exact doubling, where the legacy rule
    and the rule coincide ((2X + 1) div 4 == X div 2): that size cannot show (ii), which is why label_prep_ref.FUSION_SOURCES adds
    "0.4" (64 x 48 -> 160 x 120, a ratio of 2.5) to sampled_inputs.SOURCES."""
    P, oidx = fine_index_images(oracle)
    C, n, M = 19, 4, 64
    masks, m = _masks(size, n, M)
    assert len(set(m[(m >= 0) & (m < C)].tolist())) < ((m >= 0) & (m < C)).sum()       # no permutation

    def fused(planes):
        a = oracle.OracleAggregator(P, C, "sum", 0.5)
        for k in range(n):
            a.add(oidx[k], one_hot(planes[k], C))
        return a.get_raw().view(np.uint32)

    right = fused([lp.prepare(x, C, (si.W, si.H), m) for x in masks])
    legacy = fused([lp.prepare(x, C, (si.W, si.H), m, rule=lp.legacy_axis_index) for x in masks])
    mapped_first = fused([lp.prepare(lp.apply_map(x, m), C, (si.W, si.H)) for x in masks])
    unmapped = fused([lp.prepare(x, C, (si.W, si.H)) for x in masks])
    assert right.any()
    assert (right != legacy).any() == (size != "half")
    assert (right != unmapped).any()
    np.testing.assert_array_equal(right, mapped_first)
