"""The inputs of test_gpu_sampled.py can show a failure: checked here with resize_ref, numpy and the CPU oracle alone (no GPU).

A kernel that skipped the `sum > 0.5f` test, the re-rounding of a 16-bit source's blended row, or the border clamps of the rule
 must change the accumulator bits the GPU tests compare; these tests make sure the images and views give it the
chance.  Also: include/smesh_sampled.h against the ctypes table."""
import os
import re

import numpy as np
import pytest

import half_helpers as hh
import resize_ref as ref
import sampled_inputs as si
from helpers import small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = 15
_cache = {}


def fine_index_images(oracle):
    """The oracle's index images of test_gpu_half's "fine" scene (scene(sm, oracle, "fine") asserts the product renders the same)."""
    if "idx" not in _cache:
        mesh, cams = small_scene(a=161, b=79, views=VIEWS)
        o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
        _cache["idx"] = (len(mesh.faces), [o.render(cam)[0] for cam in cams])
    return _cache["idx"]


def visible(oidx, P):
    return np.asarray(oidx) < P


@pytest.mark.parametrize("size", sorted(si.SOURCES))
@pytest.mark.parametrize("dtype", si.DTYPES)
def test_blended_rows_fall_on_both_sides_of_the_threshold(oracle, dtype, size):
    P, oidx = fine_index_images(oracle)
    for C in (19, 40):
        small, big = si.source_images(C, dtype, si.SOURCES[size], VIEWS)
        above = below = total = 0
        for k in range(VIEWS):
            vis = visible(oidx[k], P)
            s = si.row_sums(big[k])[vis]
            above += int((s > 0.5).sum())
            below += int((~(s > 0.5)).sum())
            total += int(vis.sum())
        print("    %s %s C=%d: %d visible pixels, %.1f %% above 0.5, %.1f %% at or below" % (dtype, size, C, total, 100.0 * above / total, 100.0 * below / total))
        assert total > 0 and above >= 0.05 * total and below >= 0.05 * total


@pytest.mark.parametrize("size", sorted(si.SOURCES))
@pytest.mark.parametrize("dtype", hh.DTYPES)
def test_the_re_rounding_step_changes_the_accumulator(oracle, dtype, size):
    """The oracle fed the blended float32 rows as they are, against the oracle fed what the fusion must see: different bits."""
    P, oidx = fine_index_images(oracle)
    C, n = 19, 4
    small, big = si.source_images(C, dtype, si.SOURCES[size], VIEWS)
    with_step, without = oracle.OracleAggregator(P, C, "sum", 0.5), oracle.OracleAggregator(P, C, "sum", 0.5)
    for k in range(n):
        with_step.add(oidx[k], big[k])
        without.add(oidx[k], ref.ref_resize(small[k][1], si.W, si.H))
    a, b = with_step.get_raw().view(np.uint32), without.get_raw().view(np.uint32)
    assert a.any() and (a != b).any()


def test_visible_pixels_sit_at_every_clamped_border(oracle):
    P, oidx = fine_index_images(oracle)
    w, h = si.SOURCES["0.37"]
    x0, x1, fx = ref.axis_table(w, si.W)
    y0, y1, fy = ref.axis_table(h, si.H)
    vis = np.zeros((si.W, si.H), bool)
    for oi in oidx:
        vis |= visible(oi, P)
    # the low border: t clamped to 0, so f == 0 (i1 = 1 is never blended in); the high border: t clamped to n - 1, i1 == i0, f == 0
    xl, xh = (x0 == 0) & (fx == 0), (x1 == x0) & (x0 == w - 1)
    yl, yh = (y0 == 0) & (fy == 0), (y1 == y0) & (y0 == h - 1)
    assert (fx[xh] == 0).all() and (fy[yh] == 0).all()
    for name, rows in (("x low", vis[xl]), ("x high", vis[xh]), ("y low", vis[:, yl]), ("y high", vis[:, yh])):
        assert rows.size and rows.any(), name


def test_special_values_reach_visible_rows(oracle):
    """The planted NaN / inf / zero pixels reach visible blended rows, on both sides of the threshold test."""
    P, oidx = fine_index_images(oracle)
    for dtype in si.DTYPES:
        small, big = si.special_images(19, dtype, si.SOURCES["0.37"], 4)
        nan = zero = 0
        for k in range(4):
            vis = visible(oidx[k], P)
            rows = big[k][vis]
            nan += int(np.isnan(rows).any(axis=-1).sum())
            zero += int((rows == 0).all(axis=-1).sum())
        assert nan > 0 and zero > 0, dtype


def test_the_main_path_cases_put_every_iew_to_every_kind_and_dtype():
    """image_equal_weight 0, 0.5 and 1 each meet both kinds with all three dtypes, both class counts and every source size:
    iew = 0 is the branch where the image's weight drops out of a pixel's."""
    cases = si.main_cases()
    assert len(cases) == len(set(cases)) == 3 * 2 * 2 * 3
    assert {c[4] for c in cases} == {0.0, 0.5, 1.0}
    for dtype in si.DTYPES:
        for kind in si.KINDS:
            assert {c[4] for c in cases if c[:2] == (dtype, kind)} == {0.0, 0.5, 1.0}, (dtype, kind)
    for pos, values in ((2, (19, 40)), (3, sorted(si.SOURCES))):
        for v in values:
            assert {c[4] for c in cases if c[pos] == v} == {0.0, 0.5, 1.0}, v


def test_header_and_ctypes_table_agree():
    from semantic_meshes_amd import _lib
    text = open(os.path.join(ROOT, "include", "smesh_sampled.h")).read()
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.SAMPLED_SIGNATURES)
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.SAMPLED_SIGNATURES[name][1]), name


def test_the_keyword_needs_resize():
    """`sample_in_kernel=True` without `resize=` is refused before anything is looked at (no library needed)."""
    from semantic_meshes_amd.fusion import _MeshAggregator
    for what in ("add", "fuse_views"):
        with pytest.raises(ValueError, match="sample_in_kernel"):
            _MeshAggregator._sampling_mode(None, True, what)
    assert _MeshAggregator._sampling_mode(None, False, "add") is None
    assert _MeshAggregator._sampling_mode("bilinear", False, "add") is None
    with pytest.raises(ValueError):
        _MeshAggregator._sampling_mode("nearest", True, "add")
