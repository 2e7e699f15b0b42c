"""The tables and the preconditions of tests/test_gpu_fuse_rows_instances.py, checked without a GPU: fuse_rows_cases.py against the
CPU oracle alone.  Each precondition is a function of the scene, and is shown to FAIL on the scene that does not meet it."""
import numpy as np
import pytest

import fuse_rows_cases as fc
from fuse_rows_cases import H16, LABELS, SAMPLED


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def test_the_dispatch_as_restated():
    assert [fc.slot(C) for C in (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49)] == [8, 8, 16, 16, 24, 24, 32, 32, 40, 40, 48, 48, 0]
    assert fc.launches(15) == [8, 4, 2, 1] and fc.launches(25) == [8, 8, 8, 1] and fc.launches(11) == [8, 2, 1]
    assert fc.launches(8, 2) == [2, 2, 2, 2] and fc.launches(4, 2) == [2, 2] and fc.launches(1, 2) == [1]      # the direct rasteriser
    assert [fc.labels_form(d, C) for d, C in (("uint8", 255), ("uint16", 255), ("uint8", 256), ("uint16", 256))] == [17, 18, 1, 2]
    assert [fc.chunk(t) for t in (0, 4095, 8191, 8192, 262143, 262144, 10 ** 6)] == [1, 1, 1, 2, 63, 64, 64]
    assert fc.steps(262144) == fc.WORKERS and fc.steps(262145) == fc.WORKERS + 1


def test_the_expected_table_covers_every_instance():
    """Part A / B: TABLE reaches all 48 + 48 + 16 compiled instances and nothing else, one case each; every dtype meets every slot
    and every view count, every image_equal_weight every kernel, the class counts the low edge, the high edge and a remainder of 5
    of the slots."""
    assert len(fc.ALL_INSTANCES) == 48 + 48 + 16 == len(fc.TABLE)
    seen = [fc.instance(c) for c in fc.TABLE]
    assert len(set(seen)) == len(seen) and set(seen) == fc.ALL_INSTANCES
    # the direct rasteriser's children: the one- and two-view instances, nothing else
    direct = {fc.instance(c, 2) for c in fc.TABLE}
    assert direct == {i for i in fc.ALL_INSTANCES if i[3] <= 2}
    for kernel in (H16, SAMPLED):
        cases = [c for c in fc.TABLE if c.kernel == kernel]
        assert all(fc.slot(c.C) == c.slot for c in cases)
        for dtype in fc.DTYPES[kernel]:
            assert {c.slot for c in cases if c.dtype == dtype} == set(fc.SLOTS)
            assert {c.views for c in cases if c.dtype == dtype} == set(fc.VIEWS)
        assert {c.iew for c in cases} == set(fc.IEWS)
        assert {c.C - c.slot for c in cases} == {-7, 0, -3}
        for s in fc.SLOTS:
            assert len({c.C for c in cases if c.slot == s}) == 3
    assert {fc.size_of(c) for c in fc.TABLE if c.kernel == SAMPLED} == set(fc.SIZES)
    labels = [c for c in fc.TABLE if c.kernel == LABELS]
    assert {(c.dtype, c.C <= 255) for c in labels} == {(d, lds) for d in ("uint8", "uint16") for lds in (True, False)}
    assert {c.kind for c in labels} == set(fc.KINDS) and {c.iew for c in labels} == set(fc.IEWS)
    assert len({fc.case_id(c) for c in fc.TABLE + fc.REMAINDER_TABLE}) == len(fc.TABLE) + len(fc.REMAINDER_TABLE)


def test_the_remainder_table_takes_every_piece_of_a_partial_chunk():
    """Part C: every C mod 8 for every dtype of both kernels, in the first slot (nothing ahead of the partial chunk) and in the last
    (five whole chunks ahead); 6 and 7, the only remainders with both the 8-byte and the 4-byte piece, among them."""
    for kernel in (H16, SAMPLED):
        for dtype in fc.DTYPES[kernel]:
            cases = [c for c in fc.REMAINDER_TABLE if c.kernel == kernel and c.dtype == dtype]
            assert all(c.views == 2 for c in cases)
            for s in (8, 48):
                assert sorted(c.C % 8 for c in cases if c.slot == s) == list(range(8))
            assert {c.kind for c in cases} == set(fc.KINDS) and {c.iew for c in cases} == set(fc.IEWS)
    sizes = {fc.size_of(c) for c in fc.REMAINDER_TABLE if c.kernel == SAMPLED}
    assert sizes == set(fc.SIZES)
    for size in fc.SIZES:       # nearly every view pixel blends four distinct source pixels: four piece loads at four addresses
        assert fc.four_corner_fraction(size) > 0.98


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
def one_lane_per_row(name):
    """No face's visible pixels span more than 8: nothing is SURELY queued (the GPU case asserts the queue lengths themselves)."""
    return max(fc.facts(name).span) <= 8


def tail_precondition(name, nv):
    """Part B: the launch's views queue a triangle -- and, from two views on, one that another view of the launch shows small."""
    views = fc.TAIL_VIEWS[nv]
    if nv == 1:
        return bool(fc.facts(name).big[views[0]].any())
    return len(fc.mixed_faces(name, views)) > 0


def walk_regime(name):
    """Part F: "chunks" where 1 < chunk < 64 for every possible queue length of the eight-view launch, "second step" where chunk is
    64 and some worker takes a second step, else "single"."""
    least, most = fc.entries_bounds(name)
    if 1 < fc.chunk(least) and fc.chunk(most) < fc.WAVE:
        return "chunks"
    if fc.chunk(least) == fc.WAVE and fc.steps(least) > fc.WORKERS:
        return "second step"
    return "single" if fc.chunk(most) == 1 else "mixed"


def test_fine_has_one_lane_per_row_a_partial_last_block_and_a_face_in_the_last_corner():
    sc, f = fc.scene("fine"), fc.facts("fine")
    P = len(sc.faces)
    assert (P, P % 64) == (25438, 30) and (sc.W, sc.H) == (fc.W, fc.H)
    assert one_lane_per_row("fine") and not f.big.any()
    assert not one_lane_per_row("odd")
    assert f.visible[3, P - P % 64:].any()                            # the partial last block has work in view 3: in every launch
    # part G: views 3 and 7 show a face at (W-1, H-1), and every face visible at (W-1, y >= H-8) there is small: a main wave's lane
    # loads a run of eight labels that would end past the plane, and clamps it
    for k in (3, 7):
        assert sc.oidx[k][-1, -1] < P
        assert f.corner[k].any() and not (f.corner[k] & ~f.small[k]).any()
    assert all(k in fc.LAUNCH_VIEWS[nv] for nv in (1, 2, 4, 8) for k in (3,)) and 7 in fc.LAUNCH_VIEWS[2]


def test_odd_queues_triangles_that_other_views_show_small():
    sc, f = fc.scene("odd"), fc.facts("odd")
    P = len(sc.faces)
    assert (P, P % 64) == (1406, 62)
    per_view = f.big.sum(axis=1)
    assert (per_view.min(), per_view.max()) == (5, 167)
    assert int((f.big.any(axis=0) & (f.visible & ~f.big).any(axis=0)).sum()) == 429
    for nv in fc.VIEWS:
        assert tail_precondition("odd", nv), nv
        assert not tail_precondition("fine", nv), nv               # the precondition bites: "fine" queues nothing
    assert len(fc.mixed_faces("odd", range(8))) == 379
    assert f.visible[:, P - P % 64:].any()


def stale_plane_precondition(name, nv):
    """Part E: some view of the launch SURELY queues nothing -- every face it shows is small, so a per-view decision would skip its
    index plane -- while another view queues faces that it shows."""
    f, views = fc.facts(name), list(fc.MIXED_VIEWS[nv])
    quiet = [k for k in views if not f.big[k].any() and (f.small[k] | ~f.visible[k]).all()]
    loud = [k for k in views if f.big[k].any()]
    return bool(quiet and loud and (f.big[loud].any(axis=0) & f.small[quiet].any(axis=0)).any())


def test_mixed_has_views_that_queue_nothing_beside_views_that_queue():
    sc, f = fc.scene("mixed"), fc.facts("mixed")
    assert len(sc.faces) == 1406 and f.big.sum(axis=1).tolist() == [25, 0, 46, 0, 9, 0, 5, 0]
    assert [max(f.span[k] for k in ks) for ks in ((1, 3, 5, 7), (0, 2, 4, 6))] == [3, 11]
    for nv in (2, 4, 8):
        assert stale_plane_precondition("mixed", nv) and len(fc.mixed_faces("mixed", fc.MIXED_VIEWS[nv])) >= 45
        assert not stale_plane_precondition("odd", nv)             # the precondition bites: every view of "odd" queues triangles
        assert not stale_plane_precondition("fine", nv)            # ... and no view of "fine" does
    assert min(fc.differing_fraction("mixed", k) for k in range(8)) > 0.5


def masks_hold_losers(name):
    """Part D: in every view thousands (fine2; odd2: hundreds) of faces lie hidden under a face that is visible: their fragments lose
    the depth test, and their bits must leave the coverage masks."""
    return name in fc.LAYERED and min(fc.facts(name).hidden) >= (5000 if name == "fine2" else 500)


def test_layered_scenes_have_fragments_that_lose_the_depth_test():
    assert masks_hold_losers("fine2") and masks_hold_losers("odd2")
    assert not masks_hold_losers("fine") and not masks_hold_losers("odd")
    assert len(fc.scene("fine2").faces) == 2 * 25438 and max(fc.facts("fine2").span) <= 8 and not fc.facts("fine2").big.any()
    assert fc.facts("odd2").big.any(axis=1).all()
    for name in fc.LAYERED:
        assert min(fc.differing_fraction(name, k) for k in range(8)) > 0.5


@pytest.mark.parametrize("name", ["fine", "odd", "mid"])
def test_the_decoy_planes_differ_from_the_real_ones(name):
    """Part E: the view one further round the ring, whose plane sits in a view slot before the checked call, differs from the view
    itself at more than half of the pixels (68 % at the least)."""
    worst = min(fc.differing_fraction(name, k) for k in range(8))
    assert worst > 0.5 and worst >= 0.68 - 0.005, worst
    assert fc.decoy_views([0, 7, 3]) == [1, 0, 4]


def test_the_queue_regimes():
    """Part F: "mid" has 1 < chunk < 64 whatever the rasteriser queues beyond the sure ones, "capped" 64 and a second step."""
    assert fc.entries_bounds("mid") == (55112, 8 * 25438)
    assert (fc.chunk(55112), fc.chunk(8 * 25438)) == (13, 49)
    assert walk_regime("mid") == "chunks"
    assert walk_regime("odd") == "mixed" and walk_regime("fine") == "mixed"       # the precondition bites: chunk may be 1 there
    assert fc.chunk(fc.entries_bounds("odd")[0]) == 1
    least, most = fc.entries_bounds("capped")
    assert len(fc.scene("capped").faces) == 67600 and least == 330843 and least > fc.WAVE * fc.WORKERS
    assert walk_regime("capped") == "second step" and walk_regime("mid") != "second step"
    assert len(fc.mixed_faces("mid", range(8))) > 0


# ---- the images ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [254, 255, 256])
def test_label_images_hold_the_values_round_the_dispatch_boundary(C):
    for dtype in ("uint8", "uint16"):
        imgs = fc.label_images(fc.W, fc.H, C, dtype)
        assert len(imgs) == 8 and all(i.dtype == np.dtype(dtype) and not i.flags.writeable for i in imgs)
        values = set(np.unique(np.concatenate([i.reshape(-1) for i in imgs])).tolist())
        want = {253, 254, 255} | ({256, 257, 65535} if dtype == "uint16" else set())
        assert want <= values
        assert set(range(min(C, 256))) <= values                                  # every class the dtype can name
        lab = imgs[0]
        oh = fc.one_hot(lab, C)
        assert oh.shape == (fc.W, fc.H, C) and oh.sum() == (lab.astype(np.int64) < C).sum()
        assert (oh.sum(axis=-1) == 0).any() == (np.iinfo(dtype).max >= C)         # don't-care pixels, where the dtype can name one


def test_edge_scenes_fill_their_images():
    for size, grid in fc.EDGE_SIZES.items():
        sc = fc.edge_scene(size)
        assert (sc.W, sc.H) == size and sc.W * sc.H >= 8
        for oi in sc.oidx:
            assert oi.shape == size and (oi < len(sc.faces)).mean() > 0.5
    assert {h for w, h in fc.EDGE_SIZES} & {1, 2, 3, 4, 5, 6, 7}                  # a plane with columns shorter than a run of eight


def test_builders_are_cached_and_read_only():
    assert fc.scene("odd") is fc.scene("odd") and not fc.scene("odd").oidx[0].flags.writeable
    bits, wide = fc.h16_images(fc.W, fc.H, 5, "bfloat16")
    assert not bits[0].flags.writeable and not wide[0].flags.writeable and wide[0].dtype == np.float32
    small, big = fc.sampled_images(fc.W, fc.H, 5, "float16", "0.37")
    assert big[0].shape == (fc.W, fc.H, 5) and not big[0].flags.writeable
    assert not fc.weight_images(fc.W, fc.H)[0].flags.writeable and (fc.weight_images(fc.W, fc.H)[0] == 0).any()


def test_the_reporting_options_exist_and_are_read_only():
    """"last_fuse_labels_form", "last_fuse_flagged_views" and "compute_units" cannot be set; the first two exist without a device,
    whatever ran on this thread before (0 before any launch of the three kernels).  The one test of this module that loads the
    built library, as test_raster_instances_host.test_the_report_options_are_read_only does."""
    from semantic_meshes_amd import _lib
    assert _lib.get_option("last_fuse_labels_form") in (0, 1, 2, 17, 18)
    assert 0 <= _lib.get_option("last_fuse_flagged_views") < 256
    for name in (b"last_fuse_labels_form", b"last_fuse_flagged_views", b"compute_units"):
        assert _lib.lib().smesh_set_option(name, 1) == _lib.ERR_INVALID
