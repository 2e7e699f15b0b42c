"""The labels of a class-vector image (include/smesh_probs_labels.h, fusion.argmax_labels, ConfusionMatrix.add_probs), the part
that needs no GPU: the extension header and its ctypes table, the numpy reference the GPU tests compare with, and the argument
errors of the Python layer."""
import os
import re
import subprocess

import numpy as np
import pytest

import half_helpers as hh
import probs_labels_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PL_HEADER = os.path.join(INCLUDE, "smesh_probs_labels.h")
HEADER = os.path.join(INCLUDE, "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", PL_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(PL_HEADER)
    assert declared == ["smesh_confusion_add_probs", "smesh_probs_labels"]
    assert sorted(_lib.PROBS_LABELS_SIGNATURES) == declared       # every declared symbol has its ctypes signature
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.HALF_SIGNATURES) | set(_lib.VERTEX_SIGNATURES)
              | set(_lib.EVAL_SIGNATURES) | set(_lib.LABEL_IMAGE_SIGNATURES) | set(_lib.MESHLET_SIGNATURES))
    assert not set(declared) & others
    for other in sorted(os.listdir(INCLUDE)):
        if other != "smesh_probs_labels.h":
            assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name


def test_the_profile_slot_is_the_last_free_one():
    from semantic_meshes_amd import _lib
    slot = int(re.search(r"#define\s+SMESH_PROF_PROBS_LABELS\s+(\d+)", open(PL_HEADER).read()).group(1))
    slots = int(re.search(r"#define\s+SMESH_PROF_SLOTS\s+(\d+)", open(HEADER).read()).group(1))
    assert slot == 7 == _lib.PROF_PROBS_LABELS and slot < slots
    for other in sorted(os.listdir(INCLUDE)):
        if other == "smesh_probs_labels.h":
            continue
        text = open(os.path.join(INCLUDE, other)).read()
        used = {int(v) for name, v in re.findall(r"#define\s+(SMESH_PROF_[A-Z_]+)\s+(\d+)", text) if name != "SMESH_PROF_SLOTS"}
        assert slot not in used, other
    assert slot not in (_lib.PROF_FUSE_SCATTER, _lib.PROF_FUSE_HIST, _lib.PROF_RASTER, _lib.PROF_FINALIZE, _lib.PROF_EXCHANGE,
                        _lib.PROF_CONFUSION, _lib.PROF_LABEL_IMAGES)


# ---- the reference of the GPU tests --------------------------------------------------------------------------------------------
def test_reference_equals_argmax_without_nans_and_ties():
    rng = np.random.default_rng(1)
    for C in (1, 2, 19, 64):
        p = rng.random((23, 17, C), dtype=np.float32)
        assert C == 1 or all(len(set(row.tolist())) == C for row in p.reshape(-1, C)[:50])
        lab, dc = ref.ref_labels(p)
        assert np.array_equal(lab, np.argmax(p, axis=-1)) and not dc.any()
        s = np.zeros(p.shape[:2], np.float32)
        for c in range(C):
            s = s + p[..., c]
        lab2, dc2 = ref.ref_labels(p, 0.45 * C)
        assert np.array_equal(lab2, lab) and np.array_equal(dc2, s < np.float32(0.45 * C)) and (C == 1 or (dc2.any() and not dc2.all()))


def test_reference_gives_what_the_rule_says_on_hand_written_rows():
    nan, inf = np.nan, np.inf
    cases = [
        ([0.1, 0.7, 0.7, 0.2], 1),           # the lowest class among equals
        ([0.3, 0.3, 0.3], 0),
        ([-0.0, 0.0, -1.0], 0),              # +0 and -0 are equal
        ([0.0, -0.0, -1.0], 0),
        ([-3.0, -1.0, -2.0], 1),             # all negative
        ([0.5, inf, 0.7], 1),
        ([-inf, -5.0, -7.0], 1),
        ([-inf, -inf, -inf], 0),
        ([nan, 0.9, 0.1], 0),                # a NaN r[0] is never replaced
        ([0.2, nan, 0.1], 0),                # a NaN never replaces the best
        ([0.2, nan, 0.3], 2),
        ([6e-8, 1.2e-7, 6e-8], 1),           # float16 subnormals
        ([4.0], 0),
    ]
    for row, want in cases:
        got, dc = ref.ref_labels(np.array([row], np.float32))
        assert int(got[0]) == want and not dc[0], row
        assert ref.row_label(row) == (want, False), row
    # the don't-care test: strictly below, false for a NaN sum, -0 sums are 0
    rows = np.array([[0.5, 0.25, 0.125], [0.5, 0.25, 0.25], [0.5, nan, 0.1], [-1.0, -2.0, 0.5], [inf, 0.0, -inf]], np.float32)
    lab, dc = ref.ref_labels(rows, 1.0)
    assert lab.tolist() == [0, 0, 0, 2, 0] and dc.tolist() == [True, False, False, True, False]
    # the running sum is float32 and ordered: 1 + 2^-24 + 2^-24 stays 1 from the left, and is more than 1 from the right
    tiny = np.float32(2.0 ** -24)
    row = np.array([[1.0, tiny, tiny]], np.float32)
    assert ref.ref_labels(row, np.nextafter(np.float32(1), np.float32(2)))[1][0]
    assert not ref.ref_labels(row[:, ::-1], np.nextafter(np.float32(1), np.float32(2)))[1][0]


@pytest.mark.parametrize("C", [1, 2, 3, 19, 64])
def test_planted_rows_show_their_case_and_match_the_scalar_rule(C):
    rows = ref.planted_rows(C)
    names = [n for n, _ in rows]
    assert len(set(names)) == len(names) and (C < 3 or len(names) == 12)
    for dtype in ref.DTYPES:
        for name, row in rows:
            wide = row if dtype == "float32" else hh.widen(hh.narrow(row, dtype), dtype)
            assert np.array_equal(wide, row, equal_nan=True) and np.array_equal(np.signbit(wide), np.signbit(row)), (name, dtype)
            assert ref.is_planted(name, wide), (name, dtype)
            for thr in (None, 0.9):
                lab, dc = ref.ref_labels(wide[None, :], thr)
                assert (int(lab[0]), bool(dc[0])) == ref.row_label(wide, thr), (name, dtype, thr)
    want = {"duplicate maximum": C // 3, "-0 then +0": 0, "+0 then -0": 0, "+inf": C - 1, "-inf at r[0]": C - 1, "NaN at r[0]": 0,
            "NaN later, best before": 0, "NaN later, best after": C - 1, "-inf ties": 0 if C == 3 else 3, "all equal": 0}
    for name, row in rows:
        if name in want:
            assert ref.row_label(row)[0] == want[name], name
    rng = np.random.default_rng(2)
    _, wide, planted = ref.make_probs(rng, 9, 7, C, "float16")
    assert [n for n, _, _ in planted] == names
    for name, x, y in planted:
        assert ref.is_planted(name, wide[x, y]), name
    if C > 1:
        dc = ref.ref_labels(wide, 0.9)[1]
        assert 0.15 < dc.mean() < 0.6          # about a third of the rows sums below 0.9


# ---- argument errors of the Python layer: before a device is needed ------------------------------------------------------------
def test_argmax_labels_refuses_bad_arguments_without_a_device():
    from semantic_meshes_amd import fusion
    import semantic_meshes
    assert semantic_meshes.fusion.argmax_labels is fusion.argmax_labels
    p = np.zeros((4, 3, 5), np.float32)
    for fn in (fusion.argmax_labels, fusion.argmax_labels_device):
        with pytest.raises(ValueError):
            fn(p.astype(np.int32))                                   # not a float image
        with pytest.raises(ValueError):
            fn(p.astype(np.uint16))                                  # uint16 without probs_dtype="bfloat16"
        with pytest.raises(ValueError):
            fn(p, probs_dtype="float16")                             # the array is float32
        with pytest.raises(ValueError):
            fn(p, probs_dtype="int8")
        with pytest.raises(ValueError):
            fn(p[0])                                                 # rank 2
        with pytest.raises(ValueError):
            fn(np.zeros((4, 3, 0), np.float32))                      # no class
        for bad in (0, 4):
            with pytest.raises(ValueError):
                fn(p, dont_care_label=bad)                           # a class
        with pytest.raises(ValueError):
            fn(p, dont_care_label=256)                               # uint8 cannot hold it
        with pytest.raises(ValueError):
            fn(p, dont_care_label=-1)
        with pytest.raises(ValueError):
            fn(p, dtype=np.int64)
        with pytest.raises(ValueError):
            fn(np.zeros((2, 2, 300), np.float32), dtype=np.uint8)    # too narrow for 300 classes
        with pytest.raises(ValueError):
            fn(p, dont_care_threshold=float("nan"))


def test_add_probs_refuses_bad_arguments_without_a_device():
    from semantic_meshes_amd import fusion
    cm = fusion.ConfusionMatrix.__new__(fusion.ConfusionMatrix)      # (no handle: nothing below may get as far as the library)
    cm.classes, cm.device, cm._keep, cm._h = 5, 0, [], None
    p, gt = np.zeros((4, 3, 5), np.float32), np.zeros((4, 3), np.uint8)
    bad_calls = [
        lambda: cm.add_probs(p, gt[:3]),                             # shapes differ
        lambda: cm.add_probs(p, gt.T),
        lambda: cm.add_probs(p, gt.ravel()),
        lambda: cm.add_probs(p[:, :, :4], gt),                       # a wrong class count
        lambda: cm.add_probs(p, gt.astype(np.float32)),              # a float ground truth
        lambda: cm.add_probs(p.astype(np.int16), gt),
        lambda: cm.add_probs(p.astype(np.uint16), gt),               # uint16 without probs_dtype="bfloat16"
        lambda: cm.add_probs(p, gt, probs_dtype="float16"),
        lambda: cm.add_probs(p, gt, dont_care_threshold=float("nan")),
        lambda: cm.add_probs_many([p, p], [gt]),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert cm._keep == [], k
