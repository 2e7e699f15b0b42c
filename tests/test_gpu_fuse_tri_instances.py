"""Every compiled instance of k_fuse_tri, launched and compared with the CPU oracle.

k_fuse_tri<CT, KIND, EXACT, NV> is a family of separate compilations (fusion.hip, fusion_pair.hip, fusion_multi4.hip, fusion_multi8.hip):
twelve class-count slots -- the exact instances 5 / 13 / 19 / 20 / 21 / 40 and the run-time-C instances with 8 / 16 / 24 / 32 / 40 / 48
register slots (`tri_ct` 8 / 16 / 24 / 32 / 41 / 48) --, 1 / 2 / 4 / 8 views per launch, Sum / Summax / Mul.  Register budget, LDS row block,
the medium-triangle waves and the big-triangle tail waves differ per instance.  The expected dispatch is written down ONCE below, from
DESIGN.md 3.2 and the comments of smesh_aggregator_fuse_triangles / smesh_aggregator_max_fused_views, and every launch is checked
against it through the read-only options "last_fuse_slot" / "last_fuse_views" (smesh_get_option) and the fusion profile slot.

(a) small triangles only (one lane owns each row): bit for bit against the float32 single-threaded oracle (Mul: the float64 oracle at
    1e-5), 1 / 2 / 4 / 8 views per launch, a face count that leaves a partial last block; further block tails and strided class vectors;
(b) medium and large triangles: every instance's fuse_mid_entries / fuse_big_triangles against the float64 oracle;
(c) part (a) again in child processes under SMESH_REORDER=1 and SMESH_RASTER=direct, which pick the kernel's other two row-access modes.

Durations on an MI355X (DURATIONS below): the whole module, 159 tests, 33.9 s; of that the six child runs of part (c) 2.2 - 3.5 s each
(SMESH_REORDER=1: sum 2.53, summax 2.60, mul 2.77; SMESH_RASTER=direct: sum 2.22, summax 3.45, mul 2.63), interpreter and library start-up
included; an in-process case 0.05 - 0.6 s.
"""
import ctypes
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from helpers import assert_fused_close, random_probs, small_scene
from test_gpu_labels import bits, fuse_slot_counts

pytestmark = pytest.mark.gpu

# Measured on an MI355X (seconds): the six child runs of part (c) and the whole module.  A child's timeout is three times its
# duration, rounded up to 10 s.
DURATIONS = {
    ("SMESH_REORDER=1", "sum"): 2.53, ("SMESH_REORDER=1", "summax"): 2.60, ("SMESH_REORDER=1", "mul"): 2.77,
    ("SMESH_RASTER=direct", "sum"): 2.22, ("SMESH_RASTER=direct", "summax"): 3.45, ("SMESH_RASTER=direct", "mul"): 2.63,
    "module": 33.9,
}
CHILD_TIMEOUT = {key: int(-(-3 * d // 10) * 10) for key, d in DURATIONS.items() if key != "module"}

# both edges of every run-time slot, every exact instance, tails of 1, 2 and 3 floats, and the first count beyond the kernel
CLASSES = [1, 5, 8, 9, 13, 16, 17, 19, 20, 21, 22, 24, 25, 32, 33, 39, 40, 41, 48, 49]
KINDS = ["sum", "summax", "mul"]
SLOT_LOW_EDGES = [1, 9, 17, 25, 33, 41]                           # the most unused register slots of each run-time instance
CHILD_CLASSES = [5, 8, 13, 16, 19, 20, 21, 24, 32, 39, 40, 48]    # one class count per slot
KNOBS = ["SMESH_REORDER=1", "SMESH_RASTER=direct"]

# ---- the expected dispatch (never read back from the library) ---------------------------------------------------------------------
EXACT = (5, 13, 19, 20, 21, 40)
SLOTS = EXACT + (8, 16, 24, 32, 41, 48)
# the direct rasteriser renders one view at a time, and fuse_views then fuses its views two by two (raster.hip, fuse_views_impl)
GROUP_CAP = 2 if os.environ.get("SMESH_RASTER") == "direct" else 8


def slot(C):
    """The `tri_ct` of C classes: the class count itself for an exact instance, else the tag of the smallest run-time-C instance that
    holds it (41: the one with 40 register slots); 0 beyond k_fuse_tri."""
    if C in EXACT:
        return C
    for limit, tag in ((8, 8), (16, 16), (24, 24), (32, 32), (40, 41), (48, 48)):
        if C <= limit:
            return tag
    return 0


def views_cap(C, kind):
    """Views one launch takes: eight, except Mul at 41 .. 48 classes (the 48-slot k_fuse_tri has no registers left for more than two,
    and Mul does not move to k_fuse_tri_any)."""
    return 2 if 40 < C <= 48 and kind == "mul" else 8


def expected_launches(C, kind, n, group_cap=GROUP_CAP):
    """[(last_fuse_slot, last_fuse_views)] of one fuse_views call of n views, in order: per raster group of eight the largest of
    8 / 4 / 2 / 1 views that fits what is left; k_fuse_tri runs iff C <= 48 and not (C > 40 and more than two views)."""
    out = []
    for start in range(0, n, 8):
        left = min(8, n - start)
        while left:
            nv = 1
            while nv * 2 <= min(views_cap(C, kind), group_cap, left):
                nv *= 2
            k_fuse_tri = C <= 48 and not (C > 40 and nv > 2)
            out.append((slot(C) if k_fuse_tri else 0, nv))
            left -= nv
    return out


# every instance the dispatch allows: each slot at 1 / 2 / 4 / 8 views, the 48-slot instances at one and two views only
ALL_INSTANCES = {(kind, s, nv) for kind in KINDS for s in SLOTS for nv in (1, 2, 4, 8) if s != 48 or nv <= 2}


def last_fuse(sm):
    """("last_fuse_slot", "last_fuse_views") of the calling thread's last triangle-order launch."""
    out = []
    for name in (b"last_fuse_slot", b"last_fuse_views"):
        v = ctypes.c_int64(-7)
        sm._lib.check(sm._lib.lib().smesh_get_option(name, ctypes.byref(v)))
        out.append(int(v.value))
    return tuple(out)


def test_the_expected_table_covers_every_instance():
    """The suite's own sanity: CLASSES x KINDS x (1, 2, 4, 8) views reaches all 12 x 4 x 3 instances the dispatch allows, Sum / Summax
    at 41 .. 48 classes and everything at 49 reporting slot 0 beyond them."""
    seen = {(kind,) + expected_launches(C, kind, nv, 8)[-1] for C in CLASSES for kind in KINDS for nv in (1, 2, 4, 8)}
    assert len(ALL_INSTANCES) == 12 * 4 * 3 - 2 * 3
    assert seen - ALL_INSTANCES == {(kind, 0, nv) for kind in KINDS for nv in (1, 2, 4, 8)}
    assert ALL_INSTANCES <= seen
    assert expected_launches(48, "mul", 8, 8) == [(48, 2)] * 4 and expected_launches(41, "sum", 4, 8) == [(0, 4)]
    assert expected_launches(48, "summax", 2, 8) == [(48, 2)] and expected_launches(40, "mul", 15, 8) == [(40, 8), (40, 4), (40, 2), (40, 1)]
    assert [slot(C) for C in (1, 8, 9, 16, 17, 24, 25, 32, 33, 39, 41, 48, 49)] == [8, 8, 16, 16, 24, 24, 32, 32, 41, 41, 48, 48, 0]
    assert sorted(slot(C) for C in CHILD_CLASSES) == sorted(SLOTS)


# ---- (a) small triangles ------------------------------------------------------------------------------------------------------------
# F % 64 -> faces kept: a partial last block of 37 rows (the last 27 faces dropped), of one row (the FIRST 63 dropped: the face that
# is then alone in the last block is visible from ring position 2, none of those the grid's end leaves alone is), and none (the control)
SMALL_FACES = {37: slice(0, 6373), 1: slice(63, 6400), 0: slice(0, 6400)}
OBSERVED = set()                                # (kind, last_fuse_slot, last_fuse_views) seen by part (a) in this process
RAN = set()                                     # (C, kind) of the cases of part (a) that ran in this process


@functools.lru_cache(maxsize=None)
def small_triangles(tail):
    """The scene of test_fuse_views_wide_rows_equal_single_calls_bit_for_bit (every box at most 8 x 8 pixels) with F % 64 == tail;
    eight views: its four cameras cycled, from ring position 2 on (the first view then has work in the partial last block).  With the
    oracle's index images (rendered once)."""
    from oracle import oracle
    mesh, cams = small_scene(80, 40, 200, 150, views=4)
    faces = np.ascontiguousarray(mesh.faces[SMALL_FACES[tail]])
    assert len(faces) % 64 == tail
    o = oracle.OracleRenderer(mesh.vertices, faces)
    oidx = [o.render(cam)[0] for cam in cams]
    return types.SimpleNamespace(vertices=mesh.vertices, faces=faces, cams=[cams[(k + 2) % 4] for k in range(8)],
                                 oidx=[oidx[(k + 2) % 4] for k in range(8)])


def small_inputs(C, kind, scene):
    """Eight distinct class-vector images (5 % don't-care pixels) and per-pixel weight images."""
    rng = np.random.default_rng(1000 * C + KINDS.index(kind))
    probs = [random_probs(rng, *cam.resolution, C) for cam in scene.cams]
    if kind == "mul":
        probs = [np.maximum(p, 1e-3).astype(np.float32) for p in probs]
    weights = [rng.random(cam.resolution, dtype=np.float32) for cam in scene.cams]
    return probs, weights


def assert_small_scene(r, scene):
    """What bit equality and the partial last block need, from the oracle's index images and the rasteriser's queue lengths alone."""
    P = len(scene.faces)
    for cam in scene.cams[:4]:
        r.render(cam)
        assert r.render_stats(cam, queues=True)[1][0] == 0          # no queued triangle: one lane owns each row
    touched = np.zeros(P, bool)
    for k, idx in enumerate(scene.oidx[:4]):
        touched[idx[idx < P]] = True
        if k == 0 and P % 64:
            assert touched[P - P % 64:].any()                          # the partial last block has work in the first view already
    assert touched.sum() > P // 2


def run_small(sm, oracle, C, kind, tail):
    from semantic_meshes_amd.device import to_device
    scene = small_triangles(tail)
    P = len(scene.faces)
    r = sm.render.triangles(scene)
    assert_small_scene(r, scene)
    RAN.add((C, kind))
    probs, weights = small_inputs(C, kind, scene)
    dp, dw = [to_device(p) for p in probs], [to_device(w) for w in weights]
    # Sum / Summax: the float32 single-threaded oracle (bit equality).  Mul: the float64-accumulating oracle is the yardstick
    want = {}
    oracle.set_accum_double(kind == "mul")
    try:
        oagg = oracle.OracleAggregator(P, C, kind, 0.5)
        for k in range(8):
            oagg.add(scene.oidx[k], probs[k], weights[k])
            if k + 1 in (1, 2, 4, 8):
                want[k + 1] = (oagg.get(), None if kind == "mul" else oagg.get_raw())
    finally:
        oracle.set_accum_double(False)
    for nv in (1, 2, 4, 8):
        agg = sm.fusion.MeshAggregator(P, C, kind, 0.5)
        launches, views = fuse_slot_counts(sm, lambda: agg.fuse_views(r, scene.cams[:nv], dp[:nv], dw[:nv]))
        expected = expected_launches(C, kind, nv)
        assert (launches, views) == (len(expected), nv), (C, kind, nv)
        assert last_fuse(sm) == expected[-1], (C, kind, nv)
        OBSERVED.add((kind,) + last_fuse(sm))
        dist, raw = want[nv]
        if kind == "mul":
            assert_fused_close(agg.get(), dist)
        else:
            np.testing.assert_array_equal(bits(agg.get_raw()), bits(raw), err_msg="raw, C = %d, %s, %d views" % (C, kind, nv))
            np.testing.assert_array_equal(bits(agg.get()), bits(dist), err_msg="get(), C = %d, %s, %d views" % (C, kind, nv))


@pytest.mark.parametrize("C", CLASSES, ids=lambda C: "c%02d" % C)
@pytest.mark.parametrize("kind", KINDS)
def test_small_triangles_bit_for_bit(sm, oracle, kind, C):
    """F = 6373 (99 whole blocks and one of 37 rows: the scalar LDS fill and the guarded store of `nrows < kWave`), one fuse_views call
    of the first 1 / 2 / 4 / 8 views into a fresh aggregator each: launches, views and instance as the table says; Sum / Summax
    raw accumulator and get() equal to the float32 oracle as bit patterns, Mul within 1e-5 of the float64 oracle."""
    run_small(sm, oracle, C, kind, 37)


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("C", SLOT_LOW_EDGES, ids=lambda C: "c%02d" % C)
def test_block_tails_of_the_run_time_slots(sm, oracle, C, tail):
    """The run-time-C instances at their low edge with a single row in the last block (F = 6337) and without a partial block (6400)."""
    run_small(sm, oracle, C, "sum", tail)


@pytest.mark.parametrize("C", [C for C in CLASSES if C <= 48], ids=lambda C: "c%02d" % C)
def test_strided_class_vectors_bit_equal_the_dense_ones(sm, oracle, C):
    """A network's (H,W,C) tensor seen as (W,H,C) -- strides (C, W * C, 1), no copy -- through render() + add(): k_fuse_tri reads the
    class vectors where they are (ps0, ps1), one view per launch.  Raw accumulator bit-equal to the dense images' (part (a))."""
    from semantic_meshes_amd.device import to_device
    scene = small_triangles(37)
    P = len(scene.faces)
    r = sm.render.triangles(scene)
    probs, weights = small_inputs(C, "sum", scene)
    dw = [to_device(w) for w in weights]
    dense, strided = sm.fusion.MeshAggregator(P, C, "sum", 0.5), sm.fusion.MeshAggregator(P, C, "sum", 0.5)
    dense.fuse_views(r, scene.cams, [to_device(p) for p in probs], dw)
    for k, cam in enumerate(scene.cams):
        W, H = cam.resolution
        view = to_device(np.ascontiguousarray(probs[k].transpose(1, 0, 2))).transpose(1, 0, 2)      # (H,W,C) in memory, seen as (W,H,C)
        assert view.shape == (W, H, C) and view.strides == (C, W * C, 1)
        strided.add(r.render(cam)[0], view, dw[k])
        assert sm._lib.last_add_path() == "render-records"
        assert last_fuse(sm) == (slot(C), 1)
    np.testing.assert_array_equal(bits(strided.get_raw()), bits(dense.get_raw()))


def test_every_instance_was_observed():
    """At module end: what part (a) saw through last_fuse_slot / last_fuse_views is what its cases had to show -- and, when the whole
    of part (a) ran in this process, every instance the dispatch allows."""
    assert OBSERVED == {(kind,) + expected_launches(C, kind, nv)[-1] for C, kind in RAN for nv in (1, 2, 4, 8)}
    if GROUP_CAP == 8 and RAN >= {(C, kind) for C in CLASSES for kind in KINDS}:
        assert ALL_INSTANCES <= OBSERVED
        assert {(kind, 0, nv) for kind in ("sum", "summax") for nv in (4, 8)} <= OBSERVED      # 41 .. 48 classes: k_fuse_tri_any


# ---- (b) medium and large triangles -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def medium_triangles():
    """The scene of test_fuse_views_medium_triangles: ~20 x 20-pixel triangles plus one of ~100 x 80 pixels; F = 253.  Fifteen views,
    five cameras cycled."""
    from oracle import oracle
    mesh, cams = small_scene(14, 9, 420, 310, views=5)
    extra_v = np.array([[-1.2, -0.9, 0.8], [1.2, -0.9, 0.8], [0, 1.0, 0.8]], np.float32)
    verts = np.concatenate([mesh.vertices, extra_v])
    faces = np.concatenate([mesh.faces, [[len(mesh.vertices), len(mesh.vertices) + 1, len(mesh.vertices) + 2]]]).astype(np.int32)
    assert len(faces) == 253
    o = oracle.OracleRenderer(verts, faces)
    oidx = [o.render(cam)[0] for cam in cams]
    return types.SimpleNamespace(vertices=verts, faces=faces, cams=[cams[k % 5] for k in range(15)], oidx=[oidx[k % 5] for k in range(15)])


@pytest.mark.parametrize("C", CLASSES, ids=lambda C: "c%02d" % C)
@pytest.mark.parametrize("kind", KINDS)
def test_medium_and_large_triangles(sm, oracle, kind, C):
    """fuse_mid_entries<MCT, KIND, NV> and fuse_big_triangles<CT, KIND, EXACT, NV> of every instance: one fuse_views call of fifteen
    views (launches of 8, 4, 2 and 1; the images of a camera reused) against the float64-accumulating oracle at 1e-5."""
    from semantic_meshes_amd.device import to_device
    scene = medium_triangles()
    P = len(scene.faces)
    r = sm.render.triangles(scene)
    both = False
    for cam in scene.cams[:5]:
        r.render(cam)
        q = r.render_stats(cam, queues=True)[1]
        assert q[0] > 0 and q[1] == 0                  # boxes over 8 x 8, no queue overflow
        both = both or 0 < q[3] < q[0]                 # entries of at most 256 box pixels (medium waves) and above (tail waves)
    assert both
    rng = np.random.default_rng(2000 * C + KINDS.index(kind))
    probs = [random_probs(rng, *cam.resolution, C) for cam in scene.cams[:5]]
    if kind == "mul":
        probs = [np.maximum(p, 1e-3).astype(np.float32) for p in probs]
    weights = [(rng.random(cam.resolution, dtype=np.float32) + 0.25).astype(np.float32) for cam in scene.cams[:5]]
    dp, dw = [to_device(p) for p in probs], [to_device(w) for w in weights]
    agg = sm.fusion.MeshAggregator(P, C, kind, 0.5)
    launches, views = fuse_slot_counts(sm, lambda: agg.fuse_views(r, scene.cams, [dp[k % 5] for k in range(15)], [dw[k % 5] for k in range(15)]))
    expected = expected_launches(C, kind, 15)
    assert (launches, views) == (len(expected), 15)
    assert last_fuse(sm) == expected[-1]
    oracle.set_accum_double(True)
    try:
        oagg = oracle.OracleAggregator(P, C, kind, 0.5)
        for k in range(15):
            oagg.add(scene.oidx[k], probs[k % 5], weights[k % 5])
        want = oagg.get()
    finally:
        oracle.set_accum_double(False)
    assert (want.sum(axis=1) > 0.5).sum() > P // 2
    assert_fused_close(agg.get(), want)


# ---- (c) the other two row-access modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("knob", KNOBS)
def test_other_row_access_modes_in_child_processes(knob, kind):
    """SMESH_REORDER=1 (a position -> id table: scattered rows, the verify pass, no LDS block) and SMESH_RASTER=direct (the verify pass
    with the LDS block) are read once per process: part (a) at one class count per slot in a fresh child process, same assertions
    -- one lane still owns each row and adds its pixels in mask order."""
    name, value = knob.split("=")
    env = dict(os.environ, **{name: value})
    sel = "test_small_triangles_bit_for_bit and (%s)" % " or ".join("[%s-c%02d]" % (kind, C) for C in CHILD_CLASSES)
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel,
                          "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT[(knob, kind)])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "%d passed" % len(CHILD_CLASSES) in res.stdout, res.stdout[-1000:]

