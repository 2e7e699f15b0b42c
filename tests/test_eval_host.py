"""Confusion-matrix metrics (semantic_meshes_amd/evaluation.py, include/smesh_eval.h), the part that needs no GPU: the metric
functions on small hand-written matrices, the extension header and its ctypes table."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_HEADER = os.path.join(ROOT, "include", "smesh_eval.h")
HEADER = os.path.join(ROOT, "include", "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_metrics_on_a_hand_written_matrix():
    from semantic_meshes_amd import fusion
    #              p=0 p=1 p=2 don't care
    M = np.array([[5, 1, 0, 0],
                  [2, 3, 1, 0],
                  [0, 0, 8, 0]], np.uint64)
    assert fusion.confusion_accuracy(M) == 16 / 20
    iou = fusion.confusion_iou(M)
    assert iou.dtype == np.float64 and iou.shape == (3,)
    assert np.array_equal(iou, np.array([5 / (6 + 7 - 5), 3 / (6 + 4 - 3), 8 / (8 + 9 - 8)]))
    assert fusion.confusion_mean_iou(M) == np.mean([5 / 8, 3 / 7, 8 / 9])
    # the same through the reference package's name
    import semantic_meshes
    assert semantic_meshes.fusion.confusion_accuracy(M) == 0.8 and semantic_meshes.fusion.ConfusionMatrix is fusion.ConfusionMatrix


def test_a_class_that_never_occurs_has_a_nan_iou_and_is_left_out_of_the_mean():
    from semantic_meshes_amd import fusion
    M = np.array([[4, 0, 2, 0],
                  [0, 0, 0, 0],       # class 1: never the ground truth ...
                  [1, 0, 3, 0]], np.uint64)   # ... and never predicted
    iou = fusion.confusion_iou(M)
    assert math.isnan(iou[1]) and not math.isnan(iou[0]) and not math.isnan(iou[2])
    assert iou[0] == 4 / (6 + 5 - 4) and iou[2] == 3 / (4 + 5 - 3)
    assert fusion.confusion_mean_iou(M) == (4 / 7 + 3 / 6) / 2
    # predicted but never the ground truth: a denominator, so an IoU of 0, and part of the mean
    M2 = M.copy()
    M2[0, 1] = 2
    iou2 = fusion.confusion_iou(M2)
    assert iou2[1] == 0.0 and fusion.confusion_mean_iou(M2) == (iou2[0] + 0.0 + iou2[2]) / 3


def test_the_dont_care_column_lowers_accuracy_and_iou():
    from semantic_meshes_amd import fusion
    M = np.array([[6, 0, 0],
                  [0, 4, 0]], np.uint64)
    assert fusion.confusion_accuracy(M) == 1.0 and np.array_equal(fusion.confusion_iou(M), [1.0, 1.0])
    M[1, 2] = 10                                     # ten samples of class 1 without a prediction: errors
    assert fusion.confusion_accuracy(M) == 10 / 20
    assert np.array_equal(fusion.confusion_iou(M), [1.0, 4 / 14])
    assert M[:, 2].sum() == 10                       # ("forbidden" is the caller's check of this column)


def test_an_all_zero_matrix():
    from semantic_meshes_amd import fusion
    M = np.zeros((4, 5), np.uint64)
    assert math.isnan(fusion.confusion_accuracy(M))
    assert np.isnan(fusion.confusion_iou(M)).all() and fusion.confusion_iou(M).shape == (4,)
    assert math.isnan(fusion.confusion_mean_iou(M))


def test_a_square_matrix_is_refused():
    from semantic_meshes_amd import fusion
    for bad in (np.zeros((3, 3), np.uint64), np.zeros((3, 5), np.uint64), np.zeros(12, np.uint64), np.zeros((0, 1), np.uint64)):
        for fn in (fusion.confusion_accuracy, fusion.confusion_iou, fusion.confusion_mean_iou):
            with pytest.raises(ValueError):
                fn(bad)


def test_counts_beyond_float32_keep_their_precision():
    from semantic_meshes_amd import fusion
    big = 3 * 2 ** 40
    M = np.array([[big, 1, 0], [0, big, 0]], np.uint64)
    assert fusion.confusion_accuracy(M) == (2 * big) / (2 * big + 1)


def test_eval_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", EVAL_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(EVAL_HEADER)
    assert declared == sorted(["smesh_confusion_create", "smesh_confusion_destroy", "smesh_confusion_reset", "smesh_confusion_get",
                               "smesh_confusion_add_counts", "smesh_confusion_add_labels", "smesh_aggregator_labels",
                               "smesh_confusion_add_image", "smesh_confusion_add_view", "smesh_confusion_add_views"])
    assert sorted(_lib.EVAL_SIGNATURES) == declared                # every declared symbol has its ctypes signature
    assert not set(declared) & set(_declared(HEADER))              # none of it went into the ABI the oracle implements
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.VERTEX_SIGNATURES))
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    slot = int(re.search(r"#define\s+SMESH_PROF_CONFUSION\s+(\d+)", open(EVAL_HEADER).read()).group(1))
    slots = int(re.search(r"#define\s+SMESH_PROF_SLOTS\s+(\d+)", open(HEADER).read()).group(1))
    used = {int(v) for v in re.findall(r"#define\s+SMESH_PROF_[A-Z_]+\s+(\d+)\s*/\*", open(HEADER).read())}
    assert slot == _lib.PROF_CONFUSION and slot < slots and slot not in used


def test_confusion_matrix_refuses_bad_arguments_before_it_needs_a_device():
    from semantic_meshes_amd import fusion
    for bad in (0, -3):
        with pytest.raises(ValueError):
            fusion.ConfusionMatrix(bad)
