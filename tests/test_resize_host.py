"""Class-vector images resampled to the camera's resolution (include/smesh_resize.h, fusion.resize_probs, the `resize=` keywords),
the part that needs no GPU: the extension header and its ctypes table, the numpy reference the GPU tests compare with, and the
argument errors of the Python layer."""
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
RS_HEADER = os.path.join(INCLUDE, "smesh_resize.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", RS_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(RS_HEADER)
    assert declared == ["smesh_confusion_add_probs_resized", "smesh_resize_probs", "smesh_resize_probs_labels"]
    assert sorted(_lib.RESIZE_SIGNATURES) == declared       # every declared symbol has its ctypes signature
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.HALF_SIGNATURES) | set(_lib.VERTEX_SIGNATURES)
              | set(_lib.EVAL_SIGNATURES) | set(_lib.LABEL_IMAGE_SIGNATURES) | set(_lib.MESHLET_SIGNATURES)
              | set(_lib.PROBS_LABELS_SIGNATURES))
    assert not set(declared) & others
    for other in sorted(os.listdir(INCLUDE)):
        if other != "smesh_resize.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    text = open(RS_HEADER).read()
    assert not re.search(r"#define\s+SMESH_PROF_", text)       # all eight profile slots are taken: this header takes none
    assert int(re.search(r"#define\s+SMESH_RESIZE_BILINEAR\s+(\d+)", text).group(1)) == _lib.RESIZE_BILINEAR == _lib.RESIZE_MODES["bilinear"]


# ---- the reference of the GPU tests --------------------------------------------------------------------------------------------
def test_reference_known_answers():
    src = np.array([0.0, 1.0], np.float32).reshape(2, 1, 1)
    np.testing.assert_array_equal(ref.ref_resize(src, 4, 1).ravel(), np.array([0.0, 0.25, 0.75, 1.0], np.float32))
    i0, i1, f = ref.axis_table(2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0.0, 0.25, 0.75, 0.0]
    # the identity size returns the input, NaN and infinities included
    rng = np.random.default_rng(1)
    for dtype in ref.DTYPES:
        _, wide = ref.make_source(rng, 7, 5, 3, dtype, special=True)
        assert np.isnan(wide).any() and np.isposinf(wide).any() and np.isneginf(wide).any()
        out = ref.ref_resize(wide, 7, 5)
        np.testing.assert_array_equal(out.view(np.uint32), wide.view(np.uint32))
    # constant (finite) images stay constant; a (1,1) source gives a constant output
    for value in (0.3, -7.25, 1e-30, 3e38):
        out = ref.ref_resize(np.full((5, 4, 2), value, np.float32), 13, 9)
        assert out.shape == (13, 9, 2) and (out == np.float32(value)).all()
    one = rng.random((1, 1, 6), dtype=np.float32)
    out = ref.ref_resize(one, 6, 5)
    assert out.shape == (6, 5, 6) and (out == one[0, 0]).all()
    # downscaling by two with even sizes: the mean of the two middle samples along each axis, here of an exact ramp
    ramp = np.arange(8, dtype=np.float32).reshape(8, 1, 1)
    np.testing.assert_array_equal(ref.ref_resize(ramp, 4, 1).ravel(), np.array([0.5, 2.5, 4.5, 6.5], np.float32))


@pytest.mark.parametrize("shape", [((5, 4), (13, 9)), ((4, 3), (8, 6)), ((1, 4), (3, 9)), ((13, 9), (5, 4)), ((40, 30), (81, 61)),
                                   ((37, 53), (130, 67))])
def test_reference_agrees_with_torch_interpolate(shape):
    """torch computes the source coordinates in float32 and blends with weighted sums: equal up to rounding, not to the bit."""
    import torch
    (w, h), (W, H) = shape
    rng = np.random.default_rng(w * 1000 + h)
    src = rng.random((w, h, 5), dtype=np.float32)
    t = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 1, 0)))[None]           # (1, C, h, w)
    want = torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0].numpy().transpose(2, 1, 0)
    got = ref.ref_resize(src, W, H)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("    %s -> %s: max |reference - torch| = %.3g" % ((w, h), (W, H), err))
    assert err <= 1e-5


# ---- argument errors of the Python layer: before a device is needed ------------------------------------------------------------
def test_resize_probs_and_argmax_labels_refuse_bad_arguments_without_a_device():
    from semantic_meshes_amd import fusion
    import semantic_meshes
    assert semantic_meshes.fusion.resize_probs is fusion.resize_probs
    assert semantic_meshes.fusion.resize_probs_device is fusion.resize_probs_device
    p = np.zeros((4, 3, 5), np.float32)
    for fn in (fusion.resize_probs, fusion.resize_probs_device):
        with pytest.raises(ValueError):
            fn(p, (8, 6), mode="nearest")                            # an unknown mode
        with pytest.raises(ValueError):
            fn(p, (8, 6), mode=None)
        with pytest.raises(ValueError):
            fn(p, (-8, 6))                                           # a negative size
        with pytest.raises(ValueError):
            fn(p, 8)
        with pytest.raises(ValueError):
            fn(p, (8, 6), out_dtype=np.int16)
        with pytest.raises(ValueError):
            fn(p.astype(np.int32), (8, 6))                           # not a float image
        with pytest.raises(ValueError):
            fn(p.astype(np.uint16), (8, 6))                          # uint16 without probs_dtype="bfloat16"
        with pytest.raises(ValueError):
            fn(p[0], (8, 6))                                         # rank 2
        with pytest.raises(ValueError):
            fn(np.zeros((0, 3, 5), np.float32), (8, 6))              # nothing to sample from
    for fn in (fusion.argmax_labels, fusion.argmax_labels_device):
        with pytest.raises(ValueError):
            fn(p, size=(8, 6), resize="nearest")                     # an unknown resize string
        with pytest.raises(ValueError):
            fn(p, size=(8, 6))                                       # a size without resize
        with pytest.raises(ValueError):
            fn(p, resize="bilinear")                                 # resize without a size
        with pytest.raises(ValueError):
            fn(p, size=(8, -6), resize="bilinear")                   # a negative size
        with pytest.raises(ValueError):
            fn(p, size=(8, 6), resize="bilinear", dont_care_label=2)


def test_add_probs_refuses_bad_arguments_without_a_device():
    from semantic_meshes_amd import fusion
    cm = fusion.ConfusionMatrix.__new__(fusion.ConfusionMatrix)      # (no handle: nothing below may get as far as the library)
    cm.classes, cm.device, cm._keep, cm._h = 5, 0, [], None
    p, gt = np.zeros((4, 3, 5), np.float32), np.zeros((8, 6), np.uint8)
    with pytest.raises(ValueError, match=r"ground truth must have shape \(4, 3\)"):
        cm.add_probs(p, gt)                                          # mismatched sizes without the keyword: the old message
    with pytest.raises(ValueError, match=r"ground truth must have shape \(4, 3\)"):
        cm.add_probs(p, gt, resize=None)
    bad_calls = [
        lambda: cm.add_probs(p, gt, resize="nearest"),
        lambda: cm.add_probs(p, gt, resize=1),
        lambda: cm.add_probs(p[:, :, :4], gt, resize="bilinear"),    # a wrong class count
        lambda: cm.add_probs(p, gt.astype(np.float32), resize="bilinear"),
        lambda: cm.add_probs(p, gt.ravel(), resize="bilinear"),
        lambda: cm.add_probs(p[:0], gt, resize="bilinear"),          # nothing to sample from
        lambda: cm.add_probs_many([p, p], [gt], resize="bilinear"),
        lambda: cm.add_probs_many([p], [gt], resize="cubic"),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert cm._keep == [], k


def test_aggregator_refuses_bad_arguments_without_a_device():
    from semantic_meshes_amd import fusion
    import types
    agg = fusion.MeshAggregatorSum.__new__(fusion.MeshAggregatorSum)   # (no handle: nothing below may get as far as the library)
    agg.primitives, agg.classes, agg.device, agg.defer = 10, 5, 0, True
    agg._pending, agg._handle, agg._inflight = [], None, []
    from semantic_meshes_amd import synth
    cam, r = synth.ring_camera(0, 3, 8, 6), types.SimpleNamespace(device=0, _h=None)
    assert cam.resolution == (8, 6)
    idx, p = np.zeros((8, 6), np.uint32), np.zeros((4, 3, 5), np.float32)
    for bad in ("nearest", "Bilinear", 1, True):
        with pytest.raises(ValueError, match="resize"):
            agg.add(idx, p, resize=bad)
        with pytest.raises(ValueError, match="resize"):
            agg.add_many([idx], [p], resize=bad)
        with pytest.raises(ValueError, match="resize"):
            agg.fuse_view(r, cam, p, resize=bad)
        with pytest.raises(ValueError, match="resize"):
            agg.fuse_views(r, [cam], [p], resize=bad)
    # mismatched sizes without the keyword: the reference's message, as before
    with pytest.raises(ValueError, match="must have the same width and height"):
        agg.add(idx, p)
    with pytest.raises(ValueError, match="must have the same width and height"):
        agg.add(idx, p, resize=None)
    with pytest.raises(ValueError, match=r"probs image must be float32, float16 or bfloat16 \(W,H,C\)"):
        agg.fuse_view(r, cam, p)
    with pytest.raises(ValueError, match=r"probs image 0 must be float32, float16 or bfloat16 \(W,H,C\)"):
        agg.fuse_views(r, [cam], [p])
    with pytest.raises(ValueError):
        agg.fuse_views(r, [cam, cam], [p], resize="bilinear")     # one image per camera
    assert agg._pending == []
