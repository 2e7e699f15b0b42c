"""Compact per-triangle records (option "compact_records", semantic_meshes_amd/csrc/records.hpp) against the 16-byte TriFrag records:
one renderer, the same views, fused twice in one process -- option 0 (A) and option 1 (B).

What must hold: the raw accumulators are bit-equal, and the B side's raster launches really left the format the scene is about
("last_record_format": 8, or 16 where the launch is outside the format's scope) -- comparing the 16-byte path with itself would prove
nothing.

Class vectors.  Scenes whose triangles all stay within 8 x 8 pixels use arbitrary float32 class vectors: every accumulator row then
sees one order of additions, and bit-equality also pins that order (the 36-bit mask is walked in the 64-bit mask's pixel order).
Scenes with queued triangles (boxes over 8 x 8) use class vectors that are multiples of 1/64 and images_equal_weight = 0 (every pixel
weighs exactly 1): the float atomics of queued triangles land in no fixed order in EITHER format, and with such values every partial
sum is exact (below 2^18), so the sums are bit-equal exactly when the two formats name the same pixels: one pixel more or less on
either side still changes them.

Which kind a triangle's record gets is worked out on the host, from the cameras and the vertices, by the rasteriser's own box rule
(first / last sample column and row of the projected vertices), so that a scene asserts the branch it was built for.
"""
import numpy as np
import pytest

from helpers import random_probs
from semantic_meshes_amd import data, synth

pytestmark = pytest.mark.gpu

GROUPS = [(3, 5), (8, 19)]        # (views per fuse_views call, classes)
W, H = 160, 120


@pytest.fixture
def records_option(sm):
    """set(v) switches "compact_records"; the value found is restored."""
    before = sm._lib.get_option("compact_records")
    yield lambda v: sm._lib.set_option("compact_records", v)
    sm._lib.set_option("compact_records", before)


def fine_grid(a=100, b=15):
    """3 000 triangles = 46 x 64 + 56: the last 64-triangle block of k_fuse_tri is partial (and the last 256-triangle block of the rasteriser)."""
    return synth.grid_mesh(a, b)


def ring(n, scale=0.62, w=W, h=H):
    return [synth.ring_camera(k, n, w, h, radius_scale=scale) for k in range(n)]


def boxes(mesh, cam):
    """(bw, bh, on) per face: the size of the rasteriser's box (setup_tri: sample centres at +0.5, clamped to the image) and whether the
    triangle is in front of the camera with a non-empty box.  Vertices in float32 in the vertex stage's order, the division in double."""
    R, t = np.asarray(cam.rotation, np.float32), np.asarray(cam.translation, np.float32)
    v = np.asarray(mesh.vertices, np.float32)
    w, h = (int(x) for x in cam.resolution)
    pc = [((R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2]) + t[i] for i in range(3)]
    z = pc[2].astype(np.float64)
    fx, fy = (float(x) for x in cam.focal_lengths)
    cx, cy = (float(x) for x in cam.principal_point)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * (pc[0].astype(np.float64) / z) + cx
        s = fy * (pc[1].astype(np.float64) / z) + cy
    f = np.asarray(mesh.faces)
    front = (pc[2] > np.float32(1e-6))[f].all(axis=1)
    u, s = np.where(front[:, None], u[f], 0.0), np.where(front[:, None], s[f], 0.0)
    x0, x1 = np.maximum(np.ceil(u.min(1) - 0.5), 0), np.minimum(np.floor(u.max(1) - 0.5), w - 1)
    y0, y1 = np.maximum(np.ceil(s.min(1) - 0.5), 0), np.minimum(np.floor(s.max(1) - 0.5), h - 1)
    bw, bh = (x1 - x0 + 1).astype(np.int64), (y1 - y0 + 1).astype(np.int64)
    return bw, bh, front & (bw > 0) & (bh > 0)


def kinds(mesh, cam):
    """The compact kind the box rule gives every face (0 where it is off screen; a small triangle that covers no sample centre also gets 0
    on the device, which this does not model: the scenes assert presence, with hundreds to spare)."""
    bw, bh, on = boxes(mesh, cam)
    k = np.where((bw > 8) | (bh > 8), 2, np.where((bw > 6) | (bh > 6), 3, 1))
    return np.where(on, k, 0)


def host_probs(cams, C, seed, exact):
    rng = np.random.default_rng(seed)
    out = []
    for cam in cams:
        w, h = (int(x) for x in cam.resolution)
        p = random_probs(rng, w, h, C)
        if exact:
            p = (np.round(p * 64.0) / 64.0).astype(np.float32)
        out.append(p)
    return out


def fuse_both(sm, set_option, renderer, P, C, cams, probs, exact=False, kind="sum", expect=8, fuse=None):
    """{0: raw, 1: raw} of fuse_views(cams) with the option off and on; the format the last raster launch of each side left is asserted:
    16 on the A side, `expect` on the B side.  `exact`: `probs` are host_probs(exact=True) -- every pixel weighs 1."""
    from semantic_meshes_amd.device import to_device
    dev = [to_device(p) for p in probs]
    raws = {}
    for opt in (0, 1):
        set_option(opt)
        agg = sm.fusion.MeshAggregator(P, C, kind, 0.0 if exact else 0.5)
        if fuse is None:
            agg.fuse_views(renderer, cams, dev)
        else:
            fuse(agg, renderer, cams, dev)
        raws[opt] = agg.get_raw()
        fmt = sm._lib.get_option("last_record_format")
        assert fmt == (16 if opt == 0 else expect), (opt, fmt)
    return raws


def assert_same(raws):
    assert raws[1].any()
    assert np.array_equal(raws[0].view(np.uint32), raws[1].view(np.uint32))


@pytest.mark.parametrize("n,C", GROUPS)
def test_small_boxes_compact_words_only(sm, oracle, records_option, n, C):
    """(a) Every box at most 6 x 6: the launch reads and writes 8-byte words alone.  Arbitrary float32; also against the oracle."""
    from helpers import assert_fused_close
    mesh, cams = fine_grid(), ring(n)
    P = len(mesh.faces)
    assert P % 64 != 0 and P % 256 != 0
    ks = [kinds(mesh, cam) for cam in cams]
    assert all(set(np.unique(k)) <= {0, 1} for k in ks) and all((k == 1).sum() > 1000 for k in ks)
    r = sm.render.triangles(mesh)
    probs = host_probs(cams, C, 21, exact=False)
    assert_same(fuse_both(sm, records_option, r, P, C, cams, probs))
    agg = sm.fusion.MeshAggregator(P, C)
    from semantic_meshes_amd.device import to_device
    agg.fuse_views(r, cams, [to_device(p) for p in probs])
    o_r, o_a = oracle.OracleRenderer(mesh.vertices, mesh.faces), oracle.OracleAggregator(P, C)
    for cam, p in zip(cams, probs):
        o_a.add(o_r.render(cam)[0], p)
    assert_fused_close(agg.get(), o_a.get())


WIDE_SCALE = 0.34                  # ring cameras this close: boxes of 3 .. 8 pixels; a ring of three has none over 8, the steeper views of a ring
                                   # of eight have a few (medium triangles: queued)


def queued(mesh, cams):
    """How many (triangle, view) pairs have a box over 8 x 8.  Any at all: the scene takes exact class vectors (the module's docstring)."""
    return int(sum((kinds(mesh, cam) == 2).sum() for cam in cams))


@pytest.mark.parametrize("n,C", GROUPS)
def test_boxes_of_six_seven_and_eight_pixels(sm, records_option, n, C):
    """(b) Boxes of exactly 6, 7 and 8 pixels in x in one view and in y in another: kind 3 beside kind 1 in the same waves."""
    mesh, cams = fine_grid(), ring(n, WIDE_SCALE)
    P = len(mesh.faces)
    sizes = [boxes(mesh, cam) for cam in cams]
    in_x = [all(((bw == s) & (bh <= 8) & on).sum() > 0 for s in (6, 7, 8)) for bw, bh, on in sizes]
    in_y = [all(((bh == s) & (bw <= 8) & on).sum() > 0 for s in (6, 7, 8)) for bw, bh, on in sizes]
    assert any(in_x) and any(in_y) and any(x != y for x, y in zip(in_x, in_y)), (in_x, in_y)
    ks = [kinds(mesh, cam) for cam in cams]
    print("kind 1 / 3 / 2 per view:", [((k == 1).sum(), (k == 3).sum(), (k == 2).sum()) for k in ks])
    assert all((k == 1).sum() > 100 for k in ks) and sum((k == 3).sum() for k in ks) > 100
    exact = queued(mesh, cams) > 0
    assert exact == (n == 8)                                           # three views: nothing queued -- arbitrary float32, one order of additions
    # both kinds inside one 64-triangle block of some view
    assert any(((k.reshape(-1)[:P // 64 * 64].reshape(-1, 64) == 1).any(1) & (k.reshape(-1)[:P // 64 * 64].reshape(-1, 64) == 3).any(1)).any() for k in ks)
    r = sm.render.triangles(mesh)
    assert_same(fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 22, exact=exact), exact=exact))


def stacked(mesh, dz=0.03):
    """The grid twice, the copy dz below: wherever both are on screen the lower one loses the depth test."""
    v, f = np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces, np.int32)
    low = v.copy()
    low[:, 2] -= np.float32(dz)
    return data.Mesh(np.concatenate([v, low]), np.concatenate([f, f + len(v)]))


@pytest.mark.parametrize("n,C", GROUPS)
@pytest.mark.parametrize("scale", [0.62, WIDE_SCALE])
def test_losers_cleared_by_the_resolve(sm, oracle, records_option, n, C, scale):
    """(c) Two stacked grids: the tile resolve clears the losers' bits -- in compact words (scale 0.62: every box within 6 x 6) and in
    the TriFrag of kind-3 records as well (the closer ring).  The lower grid's visible pixels are counted with the oracle."""
    mesh, cams = stacked(fine_grid()), ring(n, scale)
    P = len(mesh.faces)
    ks = [kinds(mesh, cam) for cam in cams]
    exact = queued(mesh, cams) > 0
    assert exact == (n == 8 and scale != 0.62)
    assert (sum((k == 3).sum() for k in ks) > 100) == (scale != 0.62)
    o_r = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    idx = np.asarray(o_r.render(cams[0])[0])
    lower = int(((idx >= P // 2) & (idx < P)).sum())
    print("view 0: pixels of the lower grid that win %d, of the upper %d" % (lower, int((idx < P // 2).sum())))
    assert (idx < P // 2).sum() > 1000                                 # the upper grid hides most of the lower one: its fragments lost
    r = sm.render.triangles(mesh)
    raws = fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 23, exact=exact), exact=exact)
    assert_same(raws)
    if n == 3:
        planes = [np.asarray(o_r.render(cam)[0]) for cam in cams]
        if not any(((p >= P // 2) & (p < P)).any() for p in planes):   # the lower grid shows in no view: all its fragments lost and were
            assert not raws[1][P // 2:].any()                          # cleared -- its rows stay zero
            print("the lower grid's rows are all zero")


def with_floating_triangle(mesh, at=1500, edge=0.15, z=1.0):
    """The grid plus one horizontal triangle above its centre, inserted in the middle of the face list."""
    v, f = np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces, np.int32)
    V = len(v)
    extra_v = np.array([[-0.5 * edge, -0.4 * edge, z], [0.5 * edge, -0.4 * edge, z], [0.0, 0.6 * edge, z]], np.float32)
    return data.Mesh(np.concatenate([v, extra_v]), np.concatenate([f[:at], np.array([[V, V + 1, V + 2]], np.int32), f[at:]]))


def camera_above(height):
    """Looks down at the floating triangle from `height` above it."""
    eye = np.array([0.03, 0.02, 1.0 + height])
    R, t = synth.look_at(eye, (0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0))
    f = 0.8 * W
    return data.Camera(R, t, np.asarray([W, H]), np.asarray([f, f], np.float64), np.asarray([W / 2.0, H / 2.0], np.float64))


@pytest.mark.parametrize("n,C", GROUPS)
@pytest.mark.parametrize("height,large", [(1.5, False), (0.6, True)])
def test_queued_in_one_view_small_in_the_others(sm, records_option, n, C, height, large):
    """(d) A triangle over 8 x 8 in one view of the launch -- once medium (at most 256 pixels), once large -- and small in the others:
    the medium-triangle waves and the tail waves read its small views from compact words."""
    at = 1500
    mesh = with_floating_triangle(fine_grid(), at)
    P = len(mesh.faces)
    cams = ring(n - 1)
    cams.insert(1, camera_above(height))
    sizes = [boxes(mesh, cam) for cam in cams]
    bw, bh, on = sizes[1]
    assert on[at] and (bw[at] > 8 or bh[at] > 8) and (bw[at] * bh[at] > 256) == large, (bw[at], bh[at])
    others = [k for k in range(n) if k != 1]
    assert all(sizes[k][2][at] and sizes[k][0][at] <= 6 and sizes[k][1][at] <= 6 for k in others), [(sizes[k][0][at], sizes[k][1][at]) for k in others]
    print("the floating triangle: %d x %d from above, %s elsewhere" % (bw[at], bh[at], [(int(sizes[k][0][at]), int(sizes[k][1][at])) for k in others]))
    r = sm.render.triangles(mesh)
    raws = fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 24, exact=True), exact=True)
    assert_same(raws)
    assert raws[1][at].sum() >= 9.0                                    # the triangle's pixels were fused (over 8 x 8 in one view alone)


def test_queue_overflow_rechecks_the_masks(sm, records_option, monkeypatch):
    """(e) One slot per fragment sub-queue: the overflow goes through the key image, the resolve cannot name its losers and the fusion
    checks the expanded masks against the index plane."""
    monkeypatch.setenv("SMESH_FRAG_CAP", "1")
    mesh, cams = stacked(fine_grid()), ring(8, WIDE_SCALE)
    P, C = len(mesh.faces), 19
    r = sm.render.triangles(mesh)
    assert queued(mesh, cams) > 0                                      # (medium triangles in the steeper views: exact class vectors)
    overflow = fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 25, exact=True), exact=True)
    assert_same(overflow)
    monkeypatch.delenv("SMESH_FRAG_CAP")
    plain = fuse_both(sm, records_option, sm.render.triangles(mesh), P, C, cams, host_probs(cams, C, 25, exact=True), exact=True)
    assert np.array_equal(overflow[1], plain[1])                       # the same visible pixels either way


@pytest.mark.parametrize("kind,C", [("sum", 19), ("summax", 19), ("mul", 19), ("sum", 7), ("mul", 48)])
def test_aggregators_and_class_counts(sm, records_option, kind, C):
    """(f) Sum, Summax and Mul at 19 classes, a run-time-C instance (7 classes) and the 48-slot instance (Mul: the one aggregator whose
    every launch at 48 classes is k_fuse_tri), on the scene with kinds 1 and 3."""
    mesh, cams = fine_grid(), ring(8, WIDE_SCALE)
    P = len(mesh.faces)
    r = sm.render.triangles(mesh)
    # (eight views: a few medium triangles -- exact class vectors for Sum and Summax; Mul's queued triangles are fused by one wave each,
    # rows owned, in a fixed order: its logarithms are not exact and need not be)
    raws = fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 26, exact=True), exact=True, kind=kind)
    assert raws[1].any()
    assert np.array_equal(raws[0].view(np.uint32), raws[1].view(np.uint32))


def test_a_view_wider_than_the_origin_field(sm, records_option):
    """(g) A view of 8 200 x 8 pixels beside ordinary ones: its box origins do not fit 13 bits, the whole launch keeps TriFrag."""
    mesh = fine_grid()
    P, C = len(mesh.faces), 5
    cams = ring(2) + [synth.ring_camera(1, 3, 8200, 8)]
    r = sm.render.triangles(mesh)
    raws = fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 27, exact=True), exact=True, expect=16)
    assert_same(raws)
    # (and the ordinary views alone take the compact format)
    assert_same(fuse_both(sm, records_option, r, P, C, cams[:2], host_probs(cams[:2], C, 27, exact=True), exact=True, expect=8))


def test_a_kernel_outside_the_scope_keeps_trifrag(sm, records_option):
    """(h) 64 classes: k_fuse_tri_any reads the records, which therefore stay TriFrag with the option on."""
    mesh, cams = fine_grid(), ring(3)
    P, C = len(mesh.faces), 64
    r = sm.render.triangles(mesh)
    assert_same(fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 28, exact=False), expect=16))


def test_fuse_view_and_fuse_views_share_the_sides(sm, records_option):
    """One renderer through fuse_views (compact), fuse_view (compact, the single-view kernels), render() + add() (TriFrag) and fuse_views
    again: a side changes its format from launch to launch and every reader is told which one it holds."""
    mesh, cams = fine_grid(), ring(8, WIDE_SCALE)
    P, C = len(mesh.faces), 19

    def fuse(agg, r, cams, dev):
        agg.defer = False                                              # fuse_view below is smesh_fuse_view, not a deferred group of one
        agg.fuse_views(r, cams, dev)
        agg.fuse_view(r, cams[2], dev[2])
        agg.add(r.render(cams[3])[0], dev[3])
        agg.fuse_views(r, cams[:3], dev[:3])

    r = sm.render.triangles(mesh)
    assert_same(fuse_both(sm, records_option, r, P, C, cams, host_probs(cams, C, 29, exact=True), exact=True, fuse=fuse))
