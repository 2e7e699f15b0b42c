"""Every compiled instance of k_fuse_tri_labels, k_fuse_tri_h16 and k_fuse_tri_sampled, one launch each, against the CPU oracle.

The three kernels share fuse_rows.inc.hpp and are 16 + 48 + 48 separate compilations: k_fuse_tri_labels<uint8 / uint16 planes, 1 / 2 /
4 / 8 views, rows in LDS / in global memory>, and the two class-vector kernels with 8 .. 48 register slots x Sum / Summax x 1 / 2 / 4 /
8 views.  All sixteen label instances can be selected: the class count alone picks uint8 + LDS up to 255 classes and uint16 + global
rows beyond, but a dense uint8 / uint16 label image in device memory is read in place whatever the class count (narrow_plane), which
gives uint16 + LDS and uint8 + global rows.  The expected dispatch, the scenes, the images and the preconditions are
fuse_rows_cases.py's (checked without a GPU by test_fuse_rows_host.py); every launch is checked against them through
last_fuse_kernel() and the read-only options "last_fuse_slot" / "last_fuse_views" / "last_fuse_labels_form", through the fusion profile
slot (the call was exactly the launches the table says), and through "last_fuse_flagged_views" (which views had their masks flagged).

References never come from the library: oracle.OracleRenderer's index images and oracle.OracleAggregator on the exactly widened
images (half_helpers), on resize_ref's resampled images (sampled_inputs) and on one-hot images for labels.  Where no view of the
launch queues a triangle one lane owns each row, and get_raw() and get() equal the float32 oracle bit for bit; where triangles are
queued, helpers.assert_fused_close at its defaults against the float64-accumulating oracle.

(A) every instance alone, on "fine" (no queued triangle, a last block of 30 rows);
(B) the same table on "odd": the tail waves of every instance, with triangles that one view of the launch queues and another shows small;
(C) C = 1 .. 8 and 41 .. 48 -- every remainder of the partial-chunk loaders -- for every dtype, dense and based one element into its buffer;
(D) flagged masks: SMESH_FRAG_CAP so small that every view's / only some views' fragment queues overflow, on "fine2" / "odd2" (the
    two grids with a copy underneath: only fragments that lose the depth test make an unchecked mask wrong), and part (A) again in
    child processes under SMESH_RASTER=direct (which fuses its views two by two);
(E) stale planes: before EVERY checked call of this module the same kind of call, twice (the raster groups alternate between two banks
    of view slots), fuses the cameras one further round the ring into a throwaway aggregator with a renderer that never renders a
    camera otherwise, so that every view slot holds another view's plane, records and queues; 25 views (8 + 8 + 8 + 1) per kernel;
    and "mixed", where views that queue nothing share a launch with views that queue triangles which the former show small -- the
    one constellation in which a plane decision per view leaves a plane unwritten that a tail wave scans;
(F) the tail walk with 1 < chunk < 64 ("mid") and with chunk = 64 and a second step per worker ("capped");
(G) k_fuse_tri_labels at 254 / 255 / 256 classes, its clamped last run, and images of 7 x 3, 9 x 1000, 1000 x 9 and 33 x 65.

464 cases.  On an MI355X (DURATIONS below) the module takes 51.1 s; of that the one child process of part (D) 14.5 s as the first GPU
process on the machine (14.2 s within the module), interpreter and library start-up included.  The longest in-process case is
"capped" for k_fuse_tri_h16, 4.36 s (sampled 2.68 s, labels 1.82 s: the oracle's fusion of eight 2240 x 1680 views dominates, so all
three stay); "mid" takes 0.4 - 2.1 s (the first builds the images), every other case 0.03 - 0.85 s.

What each part guards was broken once, a line at a time, in a scratch build (whole module without the child):
  rest0 / rest1 swapped in load_part16 (C)             of the 160 cases of part (C) the 96 in which rest0 and rest1 differ: the four 16-bit
                                                       dtypes x two bases x the twelve class counts with C mod 8 not in {0, 4}; none of the
                                                       float32 cases, which do not go through load_part16; about 120 further 16-bit cases;
  rest.z / rest.w swapped in the float32 half of       the eight float32 cases of part (C) with C mod 8 in {3, 7} (3, 7, 43, 47, dense and
  k_fuse_tri_sampled's load_chunk (C)                  offset), the only ones that place a third element behind the 8-byte piece; no other;
  last_run = W * H - 9 (G)                             all four clamped-run cases, the twelve at 254 / 255 / 256 classes, 35 more label cases;
  the mask check skipped for view 0 (D)                30 of the 36 flagged-mask cases (not "some" on "odd2": view 0 is not flagged there).
                                                       On the single-sheet "fine" / "odd" no case noticed: nothing loses the depth test there;
  HALF views at the per-view plane level (E, B)        the three k_fuse_tri_h16 cases on "mixed".  Part (B) and the decoys on "odd" did
                                                       NOT notice: every view of "odd" queues triangles and writes its plane either way;
  q = l * (steps - 1) + step in the tail walk (F)      the six cases on "mid" and "capped", no other;
  chunk = 1 (F)                                        NO case: the walk then visits the same entries one per step -- slower, the same
                                                       sums.  Only a timing or a report of the chunk could see it: a gap still open.
"""
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

import fuse_rows_cases as fc
import half_helpers as hh
from fuse_rows_cases import H16, LABELS, SAMPLED, Case
from helpers import assert_fused_close
from test_gpu_half import oracle_raw
from test_gpu_labels import bits, fuse_slot_counts

pytestmark = pytest.mark.gpu

# Measured on an MI355X (seconds).  A child's timeout is three times its duration, rounded up to 10 s.
# (the child: measured as the first GPU process of a run, which is the slower of the two ways it was measured)
DURATIONS = {"SMESH_RASTER=direct": 14.46, "module": 51.1, "longest case": 4.36}
CHILD_TIMEOUT = {key: int(-(-3 * d // 10) * 10) for key, d in DURATIONS.items() if key.startswith("SMESH_")}

DIRECT = os.environ.get("SMESH_RASTER") == "direct"
GROUP_CAP = 2 if DIRECT else 8                  # the direct rasteriser hands its views over two by two
KW = {"resize": "bilinear", "sample_in_kernel": True}
OBSERVED = set()                                # fuse_rows_cases.instance of the last launch of every case of part (A) in this process
RAN = set()                                     # the cases of part (A) that ran in this process
_cache = {}


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
def renderers(sm, sc):
    """(the renderer of the decoy and the checked calls, which never renders a camera otherwise; a second one for render_stats and
    for whatever else renders a camera alone)."""
    if ("r", sc.name) not in _cache:
        mesh = types.SimpleNamespace(vertices=np.array(sc.vertices), faces=np.array(sc.faces))
        _cache["r", sc.name] = (sm.render.triangles(mesh), sm.render.triangles(mesh))
    return _cache["r", sc.name]


def stats(sm, sc, cap=""):
    """render_stats' queue lengths [boxes over 8 x 8, overflow flag, ...] of every camera of the scene, rendered alone by the second
    renderer under the SMESH_FRAG_CAP in force (`cap`: the cache key)."""
    assert os.environ.get("SMESH_FRAG_CAP", "") == cap
    if ("q", sc.name, cap) not in _cache:
        r2 = renderers(sm, sc)[1]
        out = []
        for cam in sc.cams:
            r2.render(cam)
            out.append(tuple(r2.render_stats(cam, queues=True)[1]))
        _cache["q", sc.name, cap] = tuple(out)
    return _cache["q", sc.name, cap]


def entries(sm, sc, views):
    """Queue entries of a launch of `views`: the queue lengths, each capped by the capacity (one entry per face)."""
    q = stats(sm, sc)
    return sum(min(q[k][0], len(sc.faces)) for k in views)


def inputs(sm, case, sc, views, offset, distinct):
    """(what the oracle sees of every view, the device images as a caller would hand them over)."""
    from semantic_meshes_amd.device import DeviceArray, to_device
    pick = [k % distinct for k in views]

    def device(values):
        if offset:       # based one element into its buffer: 2-byte (float32: 4-byte) alignment of every piece load
            flat = np.asarray(values).reshape(-1)
            buf = to_device(np.concatenate([flat[:1], flat]))
            d = DeviceArray(buf.ptr + flat.itemsize, values.shape, values.dtype, 0, owner=buf)
        else:
            d = to_device(values)
        d.bfloat16 = case.dtype == "bfloat16"
        return d

    if case.kernel == LABELS:
        imgs = fc.label_images(sc.W, sc.H, case.C, case.dtype)
        hot = {k: fc.one_hot(imgs[k], case.C) for k in set(pick)}
        return [hot[k] for k in pick], [device(imgs[k]) for k in pick]
    if case.kernel == H16:
        img, wide = fc.h16_images(sc.W, sc.H, case.C, case.dtype, distinct)
        return [wide[k] for k in pick], [device(hh.typed(img[k], case.dtype)) for k in pick]
    small, big = fc.sampled_images(sc.W, sc.H, case.C, case.dtype, fc.size_of(case), distinct)
    return [big[k] for k in pick], [device(small[k][0]) for k in pick]


def fuse(case, agg, r, cams, dev, dw):
    if case.kernel == LABELS:
        agg.fuse_views_labels(r, cams, dev, dw)
    elif case.kernel == H16:
        agg.fuse_views(r, cams, dev, dw, **hh.kw(case.dtype))
    else:
        agg.fuse_views(r, cams, dev, dw, **KW)


def reported(sm, case):
    """fuse_rows_cases.instance as the library reports the calling thread's last launch."""
    kernel, views = sm._lib.last_fuse_kernel(), sm._lib.get_option("last_fuse_views")
    if case.kernel == LABELS:
        assert sm._lib.get_option("last_fuse_slot") == 0
        return (kernel, sm._lib.get_option("last_fuse_labels_form"), None, views)
    return (kernel, sm._lib.get_option("last_fuse_slot"), case.kind, views)


def run(sm, oracle, case, sc, views, offset=False, distinct=8, queued=None):
    """One fuse_views call of `views` (indices into the scene's cameras) behind its decoys, checked as the module docstring says.
    Returns what the preconditions of the parts need: the flagged views of the last launch and the queue entries of the call."""
    from semantic_meshes_amd.device import to_device
    P = len(sc.faces)
    r = renderers(sm, sc)[0]
    queued = entries(sm, sc, views) if queued is None else queued
    wide, dev = inputs(sm, case, sc, views, offset, distinct)
    # a weights image on every second view of a 16-bit launch; label and sampled calls take them for every view or for none (a mixed
    # label list is fused view by view, a mixed sampled one refused): every second case has them on all its views
    if case.kernel == H16:
        weights = [fc.weight_images(sc.W, sc.H)[k % distinct] if j % 2 == 0 else None for j, k in enumerate(views)]
    else:
        weights = [fc.weight_images(sc.W, sc.H)[k % distinct] for k in views] if (case.C + len(views)) % 2 == 0 else None
    dw = None if weights is None else [None if w is None else to_device(w) for w in weights]
    for _ in range(2):       # (E) both banks of view slots, and slot 0 of a one-view call, hold the next camera's plane, records and queues
        fuse(case, sm.fusion.MeshAggregator(P, case.C, case.kind, case.iew), r, [sc.cams[k] for k in fc.decoy_views(views, len(sc.cams))], dev, dw)
    agg = sm.fusion.MeshAggregator(P, case.C, case.kind, case.iew)
    launches, fused = fuse_slot_counts(sm, lambda: fuse(case, agg, r, [sc.cams[k] for k in views], dev, dw))
    expected = fc.launches(len(views), GROUP_CAP)
    assert (launches, fused) == (len(expected), len(views)), (launches, fused, expected)
    want = fc.instance(case._replace(views=expected[-1]))
    got = reported(sm, case)
    assert got == want, (got, want)
    flagged = sm._lib.get_option("last_fuse_flagged_views")
    oidx = [sc.oidx[k] for k in views]
    raw = agg.get_raw()
    assert np.abs(raw).sum() > 0
    if queued == 0:
        want_raw, want_dist = oracle_raw(oracle, P, case.C, case.kind, case.iew, oidx, wide, weights)
        np.testing.assert_array_equal(bits(raw), bits(want_raw), err_msg="raw, " + fc.case_id(case))
        np.testing.assert_array_equal(bits(agg.get()), bits(want_dist), err_msg="get(), " + fc.case_id(case))
    else:
        want_raw, want_dist = oracle_raw(oracle, P, case.C, case.kind, case.iew, oidx, wide, weights, double=True)
        assert_fused_close(raw, want_raw)
        assert_fused_close(agg.get(), want_dist)
    return types.SimpleNamespace(flagged=flagged, queued=queued, instance=got, last_views=expected[-1])


def all_views(nv):
    return (1 << nv) - 1


# ---- (A) every instance alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.TABLE, ids=fc.case_id)
def test_every_instance_alone(sm, oracle, case):
    """One launch of 1 / 2 / 4 / 8 views of "fine" (under SMESH_RASTER=direct: launches of two views): no queued triangle, so raw
    accumulator and get() equal the float32 oracle bit for bit; the masks are flagged in no view (in every view under direct)."""
    sc = fc.scene("fine")
    views = fc.LAUNCH_VIEWS[case.views]
    out = run(sm, oracle, case, sc, views)
    assert out.queued == 0
    assert out.flagged == (all_views(out.last_views) if DIRECT else 0)
    RAN.add(case)
    OBSERVED.add(out.instance)


def test_every_instance_was_observed():
    """At the end of part (A): what the launches reported is what their cases had to show, and -- when the whole of part (A) ran in
    this process -- every compiled instance (under SMESH_RASTER=direct: every one- and two-view instance)."""
    assert OBSERVED == {fc.instance(c, GROUP_CAP) for c in RAN}
    if RAN >= set(fc.TABLE):
        assert OBSERVED == {i for i in fc.ALL_INSTANCES if i[3] <= GROUP_CAP}


# ---- (B) the tail waves of every instance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.TABLE, ids=fc.case_id)
def test_tail_waves_of_every_instance(sm, oracle, case):
    """The same table on "odd": fuse_box_rows / fuse_box_labels under for_each_queued_triangle of every instance.  From two views on
    the launch holds faces that one view surely queues and another surely does not: the tail wave scans that view's index plane --
    which the decoys have left stale wherever this call's raster launch did not write it."""
    sc = fc.scene("odd")
    views = fc.TAIL_VIEWS[case.views]
    f = fc.facts("odd")
    assert f.big[list(views)].any() and (case.views == 1 or len(fc.mixed_faces("odd", views)) > 0)
    out = run(sm, oracle, case, sc, views)
    assert out.queued >= f.big[list(views)].sum() > 0 and out.flagged == 0


# ---- (C) every remainder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [False, True], ids=["dense", "offset"])
@pytest.mark.parametrize("case", fc.REMAINDER_TABLE, ids=fc.case_id)
def test_every_remainder_of_the_partial_chunk(sm, oracle, case, offset):
    """C mod 8 = 1 .. 7 and 0 in the first and in the last slot, one launch of views 3 and 7 of "fine": load_part16 and the float32
    half of load_chunk take the 8-, 4- and 2-byte (16-, 8- and 4-byte) pieces bit by bit.  `offset`: the image starts one element
    into its buffer, so every piece is loaded at the element's own alignment."""
    out = run(sm, oracle, case, fc.scene("fine"), fc.LAUNCH_VIEWS[2], offset=offset)
    assert out.queued == 0 and out.flagged == 0


# ---- (D) flagged masks -----------------------------------------------------------------------------------------------------------------
# SMESH_FRAG_CAP (slots per fragment sub-queue): at 1 every view overflows; at the second value only some of the eight do (measured
# on an MI355X, asserted by every case from the launch's own flags)
CAPS = {"fine2": {"all": "1", "some": "896"}, "odd2": {"all": "1", "some": "1536"}}
FLAG_CASES = {LABELS: Case(LABELS, 0, "sum", 8, 19, "uint8", 0.5), H16: Case(H16, 24, "sum", 8, 19, "bfloat16", 0.5),
              SAMPLED: Case(SAMPLED, 24, "sum", 8, 19, "float16", 0.5)}


@pytest.mark.parametrize("group,nv", [("all", 1), ("all", 8), ("some", 8)], ids=["all-v1", "all-v8", "some-v8"])
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("name", ["fine2", "odd2"])
@pytest.mark.parametrize("kernel", fc.KERNELS, ids=lambda k: k[len("k_fuse_tri_"):])
def test_flagged_masks_are_checked_against_the_index_plane(sm, oracle, monkeypatch, kernel, name, kind, group, nv):
    """Fragment queues too small for a view raise its big_len[1]: every main-wave lane then re-derives its masks from the view's index
    plane -- which the decoys have left stale unless this call's render wrote it.  "all": every view of the launch is flagged;
    "some": some of the eight are and some are not (a precondition, from the launch's own flags and from render_stats of every camera
    rendered alone).  On "fine2" / "odd2": "fine" / "odd" with a copy of the grid underneath, whose fragments lose the depth test --
    on the single sheet every coverage mask is right as it stands, and skipping the check goes unnoticed.  Still the oracle's sums,
    on "fine2" bit for bit."""
    sc = fc.scene(name)
    views = fc.TAIL_VIEWS[nv] if name == "odd2" else fc.LAUNCH_VIEWS[nv]
    assert min(fc.facts(name).hidden) >= 500                        # fragments that lose the depth test: the unchecked masks are wrong
    queued = entries(sm, sc, views)                                 # (queue lengths at the default capacity)
    cap = CAPS[name][group]
    monkeypatch.setenv("SMESH_FRAG_CAP", cap)
    try:
        alone = sum(1 << j for j, k in enumerate(views) if stats(sm, sc, cap)[k][1])
        out = run(sm, oracle, FLAG_CASES[kernel]._replace(kind=kind, views=nv), sc, views, queued=queued)
        print("    cap %s: flagged views of the launch %#x, of the cameras rendered alone %#x" % (cap, out.flagged, alone))
        if group == "all":
            assert out.flagged == all_views(nv) == alone
        else:
            assert 0 < out.flagged < all_views(nv) and 0 < alone < all_views(nv)
        assert (out.queued == 0) == (name == "fine2")
    finally:
        monkeypatch.delenv("SMESH_FRAG_CAP")
        np.asarray(renderers(sm, sc)[1].render(sc.cams[0])[0])      # back to the default capacity (queues re-allocated); the second
        #                                                             renderer only: the first re-allocates with its next decoy call


def test_every_instance_under_the_direct_rasteriser_in_a_child_process():
    """SMESH_RASTER=direct (read once per process) flags the masks of every view and fuses a call's views two by two: the whole of part
    (A) in ONE fresh child process -- every one- and two-view instance of the three kernels, which kernel ran asserted from its
    report.  One child, not one per kernel: interpreter, library and HIP start-up are then paid once and are a small part of the
    measured duration that the timeout is three times of.  A child that runs out of time is reported as that, with its output so far,
    so that it cannot be mistaken for a failed assertion inside the child."""
    sel = "test_every_instance_alone or test_every_instance_was_observed"
    limit = CHILD_TIMEOUT["SMESH_RASTER=direct"]
    t0 = time.time()
    try:
        res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                             env=dict(os.environ, SMESH_RASTER="direct"), capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        so_far = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("TIMEOUT, not an assertion: the child did not finish within %d s (measured on an MI355X: %.1f s).  Its output so far:\n%s"
                    % (limit, DURATIONS["SMESH_RASTER=direct"], so_far[-3000:]))
    print("    child took %.2f s" % (time.time() - t0))
    assert res.returncode == 0, "an assertion inside the child, after %.1f s:\n" % (time.time() - t0) + res.stdout[-3000:] + res.stderr[-2000:]
    assert "%d passed" % (len(fc.TABLE) + 1) in res.stdout, res.stdout[-1000:]


# ---- (E) stale planes: 25 views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", fc.KERNELS, ids=lambda k: k[len("k_fuse_tri_"):])
def test_twenty_five_views_reuse_the_first_bank_of_view_slots(sm, oracle, kernel):
    """8 + 8 + 8 + 1 views of "odd" (its eight cameras three times round, and one): the third raster group writes the bank of view slots
    the first one used, the last view slot 0."""
    assert fc.launches(25) == [8, 8, 8, 1]
    out = run(sm, oracle, FLAG_CASES[kernel]._replace(views=25), fc.scene("odd"), [k % 8 for k in range(25)])
    assert out.queued > 0 and out.last_views == 1


@pytest.mark.parametrize("nv", [2, 4, 8])
@pytest.mark.parametrize("kernel", fc.KERNELS, ids=lambda k: k[len("k_fuse_tri_"):])
def test_views_that_queue_nothing_beside_views_that_queue(sm, oracle, kernel, nv):
    """"mixed": every second camera of "odd" three times as far away.  The far views queue nothing, so a plane decision per view would
    skip their index planes -- which the tail waves scan for the triangles that a near view of the launch queues.  In "odd" itself
    every view queues triangles and writes its plane under either decision."""
    sc, f = fc.scene("mixed"), fc.facts("mixed")
    views = fc.MIXED_VIEWS[nv]
    q = stats(sm, sc)
    assert [k for k in views if q[k][0] == 0] == [k for k in views if k % 2] and any(q[k][0] for k in views)
    assert len(fc.mixed_faces("mixed", views)) > 0
    out = run(sm, oracle, FLAG_CASES[kernel]._replace(views=nv, kind=fc.KINDS[nv % 3 % 2]), sc, views)
    assert out.queued > 0 and out.flagged == 0


# ---- (F) queue regimes ------------------------------------------------------------------------------------------------------------------
WALK_CASES = {LABELS: Case(LABELS, 0, "sum", 8, 5, "uint8", 0.5), H16: Case(H16, 8, "summax", 8, 8, "float16", 0.5),
              SAMPLED: Case(SAMPLED, 8, "sum", 8, 8, "bfloat16", 0.5)}


def compute_units(sm):
    """What the library sizes the tail blocks by (16 per unit)."""
    return sm._lib.get_option("compute_units")


@pytest.mark.parametrize("kernel", fc.KERNELS, ids=lambda k: k[len("k_fuse_tri_"):])
def test_tail_walk_in_chunks_of_several_entries(sm, oracle, kernel):
    """"mid" (25 438 faces at 960 x 720), one launch of eight views: 1 < chunk < 64 entries per step of for_each_queued_triangle, the
    regime asserted from the rasteriser's own queue lengths and the device's compute units."""
    sc = fc.scene("mid")
    total = entries(sm, sc, range(8))
    least, most = fc.entries_bounds("mid")
    assert compute_units(sm) == fc.CUS and least <= total <= most
    assert 1 < fc.chunk(total) < fc.WAVE and fc.steps(total) <= fc.WORKERS + fc.WAVE
    print("    %d queue entries: chunk %d, %d steps for %d workers" % (total, fc.chunk(total), fc.steps(total), fc.WORKERS))
    out = run(sm, oracle, WALK_CASES[kernel], sc, range(8))
    assert out.queued == total


@pytest.mark.parametrize("kernel", fc.KERNELS, ids=lambda k: k[len("k_fuse_tri_"):])
def test_tail_walk_with_a_second_step_per_worker(sm, oracle, kernel):
    """"capped" (67 600 faces at 2240 x 1680), one launch of eight views, two distinct images alternating: chunk = 64 and more steps
    than workers.  The oracle's fusion of eight such views dominates the case."""
    sc = fc.scene("capped")
    total = entries(sm, sc, range(8))
    assert compute_units(sm) == fc.CUS and total >= fc.entries_bounds("capped")[0]
    assert fc.chunk(total) == fc.WAVE and fc.steps(total) > fc.WORKERS
    print("    %d queue entries: chunk %d, %d steps for %d workers" % (total, fc.chunk(total), fc.steps(total), fc.WORKERS))
    try:
        out = run(sm, oracle, WALK_CASES[kernel], sc, range(8), distinct=2)
        assert out.queued == total
    finally:       # the two 67 600-face renderers with their 2240 x 1680 planes, and the images of that size, do not outlive the case
        for key in [k for k in _cache if k[1] == "capped"]:
            del _cache[key]
        fc.release_images()


# ---- (G) the label kernel's own edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("name", ["fine", "odd"])
@pytest.mark.parametrize("C", [254, 255, 256])
def test_labels_round_the_dispatch_boundary(sm, oracle, C, name, dtype):
    """254, 255 (an LDS block of 64 x 255 floats: 65 280 bytes) and 256 classes (rows in global memory), label values 253 .. 257, C,
    C + 1 and the dtype's largest among the data: at or above C don't care -- and still counted among the view's pixels."""
    views = fc.TAIL_VIEWS[8] if name == "odd" else fc.LAUNCH_VIEWS[8]
    case = Case(LABELS, 0, fc.KINDS[C % 2], 8, C, dtype, fc.IEWS[C % 3])
    out = run(sm, oracle, case, fc.scene(name), views)
    assert out.instance == (LABELS, np.dtype(dtype).itemsize + (16 if C <= 255 else 0), None, GROUP_CAP)
    assert (out.queued == 0) == (name == "fine")


@pytest.mark.parametrize("C,dtype", [(19, "uint8"), (19, "uint16"), (300, "uint8"), (300, "uint16")])
def test_the_clamped_last_run_of_a_label_plane(sm, oracle, C, dtype):
    """Views 3 and 7 of "fine" show small faces in the last column below row H - 8 (test_fuse_rows_host.py): their lanes load a run
    of eight labels that is clamped to the plane's end and shifted -- for uint8 and for uint16 planes, rows in LDS and in global memory."""
    f = fc.facts("fine")
    for k in (3, 7):
        assert f.corner[k].any() and not (f.corner[k] & ~f.small[k]).any()
    out = run(sm, oracle, Case(LABELS, 0, "sum", 2, C, dtype, 1.0), fc.scene("fine"), (3, 7))
    assert out.queued == 0


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("size", sorted(fc.EDGE_SIZES), ids=lambda s: "%dx%d" % s)
def test_label_images_of_odd_sizes(sm, oracle, size, dtype):
    """Planes with columns shorter than a run of eight labels (7 x 3), of one tile by sixteen and sixteen by one (9 x 1000, 1000 x 9)
    and of odd width and height (33 x 65), on meshes that fill them; two views in one launch."""
    sc = fc.edge_scene(size)
    case = Case(LABELS, 0, "summax" if dtype == "uint8" else "sum", 2, 19 if dtype == "uint8" else 300, dtype, 0.5)
    run(sm, oracle, case, sc, (0, 1))
