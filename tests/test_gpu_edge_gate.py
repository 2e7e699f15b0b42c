"""Fusion gated at occlusion edges on the GPU (include/smesh_edge_gate.h): `edge_weights` against edge_gate_ref in bits, weights and
counts, on depth planes made in numpy -- at the sizes where the kernel's tiles end, with a single nearer pixel exactly at and just
beyond the window's reach across every tile seam and image border, at the tolerance's edge, with every kind of background, in
unaligned planes and in place --; the gated fuse calls against the plain call fed the restatement's planes; the three stages in their
order; the refusals; and a shifted label image whose bleeding the gate must remove by construction."""
import ctypes

import numpy as np
import pytest

import depth_gate_ref as dg
import edge_gate_ref as eg
import view_weights_ref as vw
from helpers import assert_fused_close, random_probs, small_scene
from test_gpu_label_prep import bits, option

pytestmark = pytest.mark.gpu

C = 19
TX, TY = 32, 64                                # checked against the library's exported constants below
SHAPES = ((1, 1), (1, 37), (37, 1), (5, 3), (TX + 1, 2 * TY + 3), (2 * TX + 3, TY + 1), (67, 131),
          (40, 68))                            # the last one: H a multiple of four, the 16-byte form of the weights planes
RADII = (1, 3, 8)
FUSE_SIZES = ((96, 64), (80, 56))              # two camera resolutions inside one group
VIEWS = 9                                      # a full group of eight plus one
FAR, NEAR = np.float32(5.0), np.float32(2.0)
_cache = {}


def test_the_tile_constants_are_the_librarys(sm):
    assert (sm._lib.EDGE_TILE_X, sm._lib.EDGE_TILE_Y) == (TX, TY)


def check(sm, depth, gate_args, w_in=None, msg=""):
    """edge_weights with counts on device planes: the restatement's bits and counts, one launch.  Returns the weights."""
    from semantic_meshes_amd.device import to_device
    g, gate = eg.gate(*gate_args), sm.fusion.EdgeGate(*gate_args)
    want, want_counts = eg.weights(depth, g, w_in)
    before = option(sm, "edge_weights_launches")
    got, counts = sm.fusion.edge_weights(to_device(depth), gate, None if w_in is None else to_device(w_in), return_counts=True)
    assert option(sm, "edge_weights_launches") - before == 1
    np.testing.assert_array_equal(bits(got), bits(want), err_msg="%s %s %s" % (depth.shape, gate, msg))
    np.testing.assert_array_equal(counts, want_counts, err_msg="%s %s %s" % (depth.shape, gate, msg))
    return got, counts


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_edge_weights_equal_the_restatement(sm, shape):
    """Random planes of two depth levels plus a tenth of background, radius 1, 3 and 8 (at 5x3 the window is larger than the image),
    with and without a weights image, every flag and all of them: the bits of edge_gate_ref.weights and its counts."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    depth = eg.random_plane(rng, *shape)
    w_in = rng.uniform(0.1, 2.0, size=shape).astype(np.float32)
    seen = np.zeros(4, np.uint64)
    for radius in RADII:
        for flags in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
            for weights in (None, w_in):
                seen += check(sm, depth, (radius, 0.5, 0.0) + flags, weights)[1]
        # host planes, no counts
        got = sm.fusion.edge_weights(depth, sm.fusion.EdgeGate(radius, 0.5, 0.1, True, True, True), w_in)
        np.testing.assert_array_equal(bits(got), bits(eg.weights(depth, eg.gate(radius, 0.5, 0.1, True, True, True), w_in)[0]))
    print("    %s: counts over the gates %s" % (shape, seen))
    if shape[0] * shape[1] > 100:
        assert (seen > 0).all()


# ---- seams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_a_nearer_pixel_reaches_exactly_radius_pixels_across_seams_and_borders(sm, radius):
    """A flat plane with ONE nearer pixel at Chebyshev distance exactly r, then exactly r + 1, from a tested pixel: across the tile
    seam in x, in y and diagonally through the corner halo, in both directions, and against each image border.  The first must
    gate the tested pixel, the second must not; every plane also equals the restatement."""
    W, H = 2 * TX + 3, 2 * TY + 3
    r = radius
    cases = [((TX - 1, 10), (1, 0)), ((TX, 10), (-1, 0)),                      # the seam in x, from either side
             ((10, TY - 1), (0, 1)), ((10, TY), (0, -1)),                      # the seam in y
             ((TX - 1, TY - 1), (1, 1)), ((TX, TY), (-1, -1)), ((TX - 1, TY), (1, -1)), ((TX, TY - 1), (-1, 1)),   # the corner halo
             ((0, 20), (1, 0)), ((W - 1, 20), (-1, 0)), ((20, 0), (0, 1)), ((20, H - 1), (0, -1)),                 # each image border
             ((0, 0), (1, 1)), ((W - 1, H - 1), (-1, -1))]
    for (qx, qy), (sx, sy) in cases:
        for dist, gated in ((r, True), (r + 1, False)):
            depth = np.full((W, H), FAR, np.float32)
            px, py = qx + sx * dist, qy + sy * dist
            assert 0 <= px < W and 0 <= py < H
            depth[px, py] = NEAR
            got, counts = check(sm, depth, (r, 0.5), msg="q=%s p=%s" % ((qx, qy), (px, py)))
            assert (got[qx, qy] == 0) == gated, ((qx, qy), (px, py), dist)
            assert got[px, py] == 1                                            # behind only: the near pixel itself stays
            # exactly the visible pixels within r of the near one are behind it
            n = (min(px + r, W - 1) - max(px - r, 0) + 1) * (min(py + r, H - 1) - max(py - r, 0) + 1) - 1
            assert list(counts) == [W * H, n, 0, 0]


# ---- tolerance -------------------------------------------------------------------------------------------------------------------
def test_the_tolerance_to_the_bit(sm):
    """d - lo == t exactly is kept, one ulp above is dropped: with abs_tol alone, with rel_tol alone, and with a tolerance of zero."""
    def corner(d, lo, gate_args):
        depth = np.full((5, 5), d, np.float32)
        depth[2, 2] = lo
        return check(sm, depth, gate_args)[0][0, 0]

    d, up = np.float32(3.5), np.nextafter(np.float32(3.5), np.float32(4))
    lo, t = np.float32(0.5), np.float32(3.0)
    assert d - lo == t and up - lo == np.nextafter(t, np.float32(4))            # float32, both exact
    assert corner(d, lo, (2, 3.0)) == 1
    assert corner(up, lo, (2, 3.0)) == 0
    # rel_tol alone: t = 0.5 * d
    lo = np.float32(1.75)
    assert d - lo == np.float32(0.5) * d and up - lo > np.float32(0.5) * up
    assert corner(d, lo, (2, 0.0, 0.5)) == 1
    assert corner(up, lo, (2, 0.0, 0.5)) == 0
    # abs_tol = 0 and rel_tol = 0: equal depths stay, the smallest step drops
    assert corner(d, d, (2, 0.0)) == 1
    assert corner(up, d, (2, 0.0)) == 0
    # the same in front: hi - d
    assert corner(np.float32(0.5), np.float32(3.5), (2, 3.0, 0.0, False, True)) == 1
    assert corner(np.float32(0.5), up, (2, 3.0, 0.0, False, True)) == 0


# ---- background ------------------------------------------------------------------------------------------------------------------
def test_background_of_every_kind(sm):
    """NaN and -inf in a caller's plane are background like the rasteriser's +inf: weight 0, counted nowhere, never part of lo or hi,
    and a reason to drop their neighbours only under `silhouette`.  A pixel that is behind and at the silhouette is counted once, as
    behind."""
    for bad in (np.float32(np.nan), np.float32(-np.inf), np.float32(np.inf)):
        depth = np.full((TX + 5, TY + 5), FAR, np.float32)
        depth[TX, TY] = bad                                                    # (in the corner of four tiles)
        depth[3, 3] = bad
        # behind and front with a tolerance any finite step would exceed: -inf as lo or +inf as hi would drop the neighbours
        got, counts = check(sm, depth, (2, 0.0, 0.0, True, True, False))
        assert list(counts) == [depth.size - 2, 0, 0, 0] and got[TX, TY] == 0 and got[3, 3] == 0 and got.sum() == depth.size - 2
        got, counts = check(sm, depth, (2, 0.0, 0.0, True, True, True))
        assert list(counts) == [depth.size - 2, 0, 0, 48] and got[TX - 2, TY + 2] == 0 and got[TX - 3, TY] == 1
    # a mixture, with a weights image
    rng = np.random.default_rng(5)
    depth = eg.random_plane(rng, 67, 70)
    pick = rng.random(depth.shape)
    depth[pick < 0.02] = np.nan
    depth[pick > 0.98] = -np.inf
    w_in = rng.uniform(0.1, 2.0, size=depth.shape).astype(np.float32)
    for sil in (False, True):
        check(sm, depth, (3, 0.5, 0.0, True, True, sil), w_in)
    # precedence: [near, far, background] along y, radius 1
    got, counts = check(sm, np.array([[NEAR, FAR, np.inf]], np.float32), (1, 0.5, 0.0, True, False, True))
    assert list(got[0]) == [1, 0, 0] and list(counts) == [2, 1, 0, 0]
    got, counts = check(sm, np.array([[NEAR, FAR, np.inf]], np.float32), (1, 0.5, 0.0, False, False, True))
    assert list(got[0]) == [1, 0, 0] and list(counts) == [2, 0, 0, 1]


# ---- planes ----------------------------------------------------------------------------------------------------------------------
def test_unaligned_planes_in_place_and_the_weights_image(sm):
    """The depth, weights-in and weights-out planes each four bytes behind a 16-byte boundary (the one-by-one form; H is a multiple
    of four, so only the addresses decide); weights_out == weights_in; nothing written outside the plane; kept pixels carry w_in."""
    from semantic_meshes_amd.device import to_device
    lib = sm._lib.lib()
    shape = (TX + 8, TY + 4)
    N = shape[0] * shape[1]
    rng = np.random.default_rng(11)
    depth = eg.random_plane(rng, *shape)
    w_in = rng.uniform(0.1, 2.0, size=shape).astype(np.float32)
    args = (3, 0.5, 0.0, True, True, True)
    want, want_counts = eg.weights(depth, eg.gate(*args), w_in)
    kept = want != 0
    assert 0 < kept.sum() < np.isfinite(depth).sum()
    np.testing.assert_array_equal(bits(want)[kept], bits(w_in)[kept])
    pod = sm.fusion.EdgeGate(*args)._pod()
    pad = np.zeros(1, np.float32)
    for off in (4, 0):
        k = off // 4
        d_depth = to_device(np.concatenate([pad, depth.reshape(-1)])[1 - k:])
        d_w = to_device(np.concatenate([pad, w_in.reshape(-1)])[1 - k:])
        out = to_device(np.full(N + 2, -1.0, np.float32))
        counts = np.zeros(4, np.uint64)
        assert (d_depth.ptr + off) % 16 == off and (d_w.ptr + off) % 16 == off and (out.ptr + 4) % 16 == 4
        # (out is always one float in: with off == 0 the inputs are aligned and the output is not -- still one by one)
        sm._lib.check(lib.smesh_edge_weights(ctypes.c_void_p(d_depth.ptr + off), shape[0], shape[1], ctypes.byref(pod), ctypes.c_void_p(d_w.ptr + off),
                                             ctypes.c_void_p(out.ptr + 4), counts.ctypes.data_as(ctypes.c_void_p), 0))
        host = out.numpy()
        assert host[0] == -1.0 and host[-1] == -1.0                 # nothing written outside the plane
        np.testing.assert_array_equal(bits(host[1:-1].reshape(shape)), bits(want))
        np.testing.assert_array_equal(counts, want_counts)
        # in place, unaligned (off 4) and aligned (off 0: the 16-byte form)
        sm._lib.check(lib.smesh_edge_weights(ctypes.c_void_p(d_depth.ptr + off), shape[0], shape[1], ctypes.byref(pod), ctypes.c_void_p(d_w.ptr + off),
                                             ctypes.c_void_p(d_w.ptr + off), None, 0))
        sm._lib.check(lib.smesh_synchronize(0))
        np.testing.assert_array_equal(bits(d_w.numpy()[k:k + N].reshape(shape)), bits(want))
        np.testing.assert_array_equal(bits(d_depth.numpy()[k:k + N].reshape(shape)), bits(depth))     # the depth plane is never written


def test_all_flags_off_is_w_in_in_bits(sm):
    rng = np.random.default_rng(3)
    depth = eg.random_plane(rng, 67, 68)
    depth[5, 5] = np.nan
    w_in = rng.uniform(0.1, 2.0, size=depth.shape).astype(np.float32)
    got, counts = check(sm, depth, (8, 0.0, 0.0, False, False, False), w_in)
    visible = np.isfinite(depth)
    np.testing.assert_array_equal(bits(got), np.where(visible, bits(w_in), 0))
    assert list(counts) == [visible.sum(), 0, 0, 0]


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
GATE = (3, 0.15, 0.01, True, True, True)


def fuse_scene(sm):
    """Nine ring cameras over small_scene's mesh, alternating between two resolutions, with the render's own planes, class vectors,
    the caller's weights and uint16 sensor images of one size, a third of whose samples are off; built once and left unchanged."""
    if "fuse" not in _cache:
        from semantic_meshes_amd import synth
        mesh, _ = small_scene()
        cams = [synth.ring_camera(k, VIEWS, *FUSE_SIZES[k % 2]) for k in range(VIEWS)]
        r = sm.render.triangles(mesh)
        rng = np.random.default_rng(31)
        idx, depth, probs, mine, sensors, queued = [], [], [], [], [], 0
        for cam in cams:
            i, d = (np.array(p) for p in r.render(cam))
            queued += int(r.render_stats(cam, queues=True)[1][0])
            idx.append(i)
            depth.append(d)
            probs.append(np.maximum(random_probs(rng, *cam.resolution, C), 1e-3).astype(np.float32))
            mine.append(rng.uniform(0.1, 2.0, size=cam.resolution).astype(np.float32))
            near = d[dg.axis_index(d.shape[0], FUSE_SIZES[0][0])[:, None], dg.axis_index(d.shape[1], FUSE_SIZES[0][1])[None, :]].astype(np.float64)
            mm = np.where(np.isfinite(near), np.rint(1000.0 * near + np.where(rng.random(near.shape) < 0.3, 500.0, 0.0)), 0.0)
            sensors.append(mm.astype(np.uint16))
        _cache["fuse"] = dict(mesh=mesh, cams=cams, idx=idx, depth=depth, probs=probs, mine=mine, sensors=sensors, P=len(mesh.faces),
                              normals=vw.face_normals(mesh.vertices, mesh.faces), exact=queued == 0)
    return _cache["fuse"]


def ref_planes(sc, g, weights_in=None, depth=None):
    depth = sc["depth"] if depth is None else depth
    out = [eg.weights(depth[k], g, None if weights_in is None else weights_in[k]) for k in range(VIEWS)]
    return [w for w, _ in out], np.stack([c for _, c in out])


def same(sc, kind, got, want):
    """Bits for Sum / Summax where one lane owns every row, else the project's 1e-5 (the rule of test_gpu_view_weights.py)."""
    assert np.abs(want.get()).sum() > 0
    if kind != "mul" and sc["exact"]:
        np.testing.assert_array_equal(bits(got.get_raw()), bits(want.get_raw()))
    else:
        assert_fused_close(got.get(), want.get())


@pytest.mark.parametrize("kind", ["sum", "summax", "mul"])
def test_gated_fuse_views_is_the_plain_call_with_the_rules_weights(sm, kind):
    """Nine views -- a group of eight and one more, two resolutions inside a group -- with device class vectors and the caller's
    weights: the plain call with the restatement's planes; the same kernel, one k_edge_weights launch per group, the counts."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    Wref, counts = ref_planes(sc, eg.gate(*GATE), sc["mine"])
    print("    counts per view\n%s" % counts)
    assert (counts[:, 1:].sum(axis=1) > 0).all() and all(0 < (w > 0).sum() for w in Wref)
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C, kind)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wref])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C, kind)
    before = option(sm, "edge_weights_launches"), option(sm, "view_weights_launches"), option(sm, "depth_weights_launches")
    stats = got.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in sc["mine"]], edge_gate=sm.fusion.EdgeGate(*GATE), edge_stats=True)
    assert sm._lib.last_fuse_kernel() == kernel
    assert option(sm, "edge_weights_launches") - before[0] == 2
    assert (option(sm, "view_weights_launches"), option(sm, "depth_weights_launches")) == before[1:]
    assert stats.shape == (VIEWS, 4) and stats.dtype == np.uint64
    np.testing.assert_array_equal(stats, counts)
    same(sc, kind, got, plain)
    # host images, no stats: the same
    again = sm.fusion.MeshAggregator(sc["P"], C, kind)
    assert again.fuse_views(r, sc["cams"], sc["probs"], sc["mine"], edge_gate=sm.fusion.EdgeGate(*GATE)) is None
    same(sc, kind, again, plain)


def test_label_16_bit_per_view_and_texel_forms(sm):
    """fuse_views_labels(edge_gate=), a float16 fuse_views, render() + edge_weights_device + add() per view, and a texel renderer:
    each the plain call with the restatement's planes."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    gate, g = sm.fusion.EdgeGate(*GATE), eg.gate(*GATE)
    Wref, counts = ref_planes(sc, g)
    rng = np.random.default_rng(13)

    def twin(gated, plain, prefix, P=sc["P"], exact=True):
        a, b = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
        plain(b)
        kernel = sm._lib.last_fuse_kernel()
        gated(a)
        assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith(prefix), kernel
        if exact:
            same(sc, "sum", a, b)
        else:
            assert np.abs(b.get()).sum() > 0
            assert_fused_close(a.get(), b.get())

    half = [sm.fusion.narrow_probs(p, "float16") for p in sc["probs"]]
    twin(lambda a: a.fuse_views(r, sc["cams"], half, edge_gate=gate), lambda b: b.fuse_views(r, sc["cams"], half, [to_device(w) for w in Wref]),
         "k_fuse_tri_h16")
    masks = [rng.integers(0, C + 2, size=cam.resolution).astype(np.uint8) for cam in sc["cams"]]
    twin(lambda a: a.fuse_views_labels(r, sc["cams"], masks, edge_gate=gate), lambda b: b.fuse_views_labels(r, sc["cams"], masks, Wref),
         "k_fuse_tri_labels")
    # the per-view route
    batch, each = sm.fusion.MeshAggregator(sc["P"], C), sm.fusion.MeshAggregator(sc["P"], C)
    batch.fuse_views(r, sc["cams"], sc["probs"], edge_gate=gate)
    for k, cam in enumerate(sc["cams"]):
        idx, depth = r.render(cam)
        w, c = sm.fusion.edge_weights_device(depth, gate, return_counts=True)
        assert w.shape == cam.resolution and w.dtype == np.float32
        np.testing.assert_array_equal(c, counts[k])
        np.testing.assert_array_equal(bits(w.numpy()), bits(Wref[k]))
        each.add(idx, to_device(sc["probs"][k]), w)
    same(sc, "sum", each, batch)
    # a texel renderer: its own depth planes, the views fused one by one
    rt = sm.render.texels(sc["mesh"], sc["cams"], 0.05)
    tdepth = [np.array(rt.render(cam)[1]) for cam in sc["cams"]]
    Wt, tcounts = ref_planes(sc, g, depth=tdepth)
    before = option(sm, "edge_weights_launches")
    a = sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C)
    stats = a.fuse_views(rt, sc["cams"], sc["probs"], edge_gate=gate, edge_stats=True)
    assert option(sm, "edge_weights_launches") - before == 2 and sm._lib.last_fuse_kernel() == "k_fuse_texel"
    np.testing.assert_array_equal(stats, tcounts)
    b = sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C)
    b.fuse_views(rt, sc["cams"], [to_device(p) for p in sc["probs"]], [to_device(w) for w in Wt])
    assert np.abs(b.get()).sum() > 0
    assert_fused_close(a.get(), b.get())


def test_a_deferred_view_goes_first(sm):
    """Two deferred views, then an edge-gated fuse_view (and fuse_view_labels): the deferred views are handed over first -- the plain
    calls with the restatement's planes in the same order."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    gate = sm.fusion.EdgeGate(*GATE)
    Wref, counts = ref_planes(sc, eg.gate(*GATE))
    v = [0, 2, 4, 6, 8]                         # (these share a resolution: a deferred group holds views of one size)
    mask = np.random.default_rng(2).integers(0, C, size=sc["cams"][v[4]].resolution).astype(np.uint8)
    a = sm.fusion.MeshAggregator(sc["P"], C, "sum", 0.5)
    a.defer = True
    a.fuse_view(r, sc["cams"][v[0]], to_device(sc["probs"][v[0]]))
    a.fuse_view(r, sc["cams"][v[1]], to_device(sc["probs"][v[1]]))
    assert len(a._pending) == 2
    stats = a.fuse_view(r, sc["cams"][v[2]], sc["probs"][v[2]], edge_gate=gate, edge_stats=True)
    assert len(a._pending) == 0
    np.testing.assert_array_equal(stats, counts[v[2]])
    a.fuse_view(r, sc["cams"][v[3]], to_device(sc["probs"][v[3]]))
    assert a.fuse_view_labels(r, sc["cams"][v[4]], mask, edge_gate=gate) is None
    assert len(a._pending) == 0
    want = sm.fusion.MeshAggregator(sc["P"], C, "sum", 0.5)
    want.defer = False
    for k in v[:4]:
        want.fuse_view(r, sc["cams"][k], to_device(sc["probs"][k]), None if k != v[2] else to_device(Wref[k]))
    want.fuse_view_labels(r, sc["cams"][v[4]], mask, Wref[v[4]])
    same(sc, "sum", a, want)


# ---- order -----------------------------------------------------------------------------------------------------------------------
VSPEC = (2, 0.3, True, 7.5, 4.0)


def test_view_weights_then_edge_gate_then_depth_gate(sm):
    """All three stages: the plain call with the composition of the three restatements in the order view -> edge -> depth; every
    stats array its own stage's counts (a zero stays zero); one launch of each kernel per group; every subset of the stats."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    g, gd = eg.gate(*GATE), dg.gate(0.02, missing="drop")
    first = [vw.weights(sc["cams"][k], sc["normals"], sc["idx"][k], sc["depth"][k], vw.spec(*VSPEC), sc["mine"][k]) for k in range(VIEWS)]
    Wv, vcounts = [w for w, _ in first], np.stack([c for _, c in first])
    We, ecounts = ref_planes(sc, g, Wv)
    last = [dg.weights(sc["depth"][k], sc["sensors"][k], gd, We[k]) for k in range(VIEWS)]
    Wd, dcounts = [w for w, _ in last], np.stack([c for _, c in last])
    assert all((a != b).any() and (b != c).any() for a, b, c in zip(Wv, We, Wd))
    np.testing.assert_array_equal(ecounts, ref_planes(sc, g)[1])                  # the edge counts are those of the gate alone
    kw = dict(sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02, missing="drop"), view_weights=sm.fusion.ViewWeights(*VSPEC),
              edge_gate=sm.fusion.EdgeGate(*GATE))
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wd])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C)
    names = ("view_weights_launches", "edge_weights_launches", "depth_weights_launches")
    before = [option(sm, n) for n in names]
    stats = got.fuse_views(r, sc["cams"], d_probs, sc["mine"], view_stats=True, edge_stats=True, depth_stats=True, **kw)
    assert [option(sm, n) - b for n, b in zip(names, before)] == [2, 2, 2] and sm._lib.last_fuse_kernel() == kernel
    assert isinstance(stats, tuple) and len(stats) == 3
    for s, want in zip(stats, (vcounts, ecounts, dcounts)):
        np.testing.assert_array_equal(s, want)
    same(sc, "sum", got, plain)
    # the stats asked for, in the order (view, edge, depth); a single one bare
    a = sm.fusion.MeshAggregator(sc["P"], C)
    pair = a.fuse_views(r, sc["cams"], d_probs, sc["mine"], edge_stats=True, depth_stats=True, **kw)
    assert isinstance(pair, tuple) and len(pair) == 2
    np.testing.assert_array_equal(pair[0], ecounts)
    np.testing.assert_array_equal(pair[1], dcounts)
    same(sc, "sum", a, plain)
    # two stages: edge -> depth without view weights, view -> edge without a depth gate
    for drop, Wwant in (("view_weights", [dg.weights(sc["depth"][k], sc["sensors"][k], gd, ref_planes(sc, g, sc["mine"])[0][k])[0] for k in range(VIEWS)]),
                        ("depth_gate", We)):
        kw2 = {k: v for k, v in kw.items() if k != drop and not (drop == "depth_gate" and k == "sensor_depths")}
        a, b = sm.fusion.MeshAggregator(sc["P"], C), sm.fusion.MeshAggregator(sc["P"], C)
        only = a.fuse_views(r, sc["cams"], d_probs, sc["mine"], edge_stats=True, **kw2)
        np.testing.assert_array_equal(only, ecounts)
        b.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wwant])
        same(sc, "sum", a, b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(sm):
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    rt = sm.render.texels(sc["mesh"], sc["cams"], 0.05)
    gate = sm.fusion.EdgeGate(*GATE)
    a = sm.fusion.MeshAggregator(sc["P"], C)
    a.fuse_view(r, sc["cams"][0], sc["probs"][0], edge_gate=gate)
    before = bits(a.get_raw()).copy()
    assert before.any()
    a.fuse_view(r, sc["cams"][1], to_device(sc["probs"][1]))       # one deferred view: a refused call must leave it pending
    assert len(a._pending) == 1
    launches = option(sm, "edge_weights_launches")
    cams, probs, sensors = sc["cams"][2:4], sc["probs"][2:4], sc["sensors"][2:4]
    dgate, spec = sm.fusion.DepthGate(0.02), sm.fusion.ViewWeights(2, 0.3)
    for call in (lambda: a.fuse_views(r, cams, probs, edge_gate=(3, 0.1)),
                 lambda: a.fuse_views(r, cams, probs, edge_stats=True),
                 lambda: a.fuse_views(r, cams, probs, edge_gate=gate, depth_stats=True),
                 lambda: a.fuse_views(r, cams, probs, edge_gate=gate, view_stats=True),
                 lambda: a.fuse_views(r, cams, probs, edge_gate=gate, sensor_depths=sensors),
                 lambda: a.fuse_views(r, cams, probs, edge_gate=gate, sensor_depths=sensors[:1], depth_gate=dgate),
                 lambda: a.fuse_views(r, cams, probs, resize="bilinear", sample_in_kernel=True, edge_gate=gate),
                 lambda: a.fuse_view(r, cams[0], probs[0], resize="bilinear", sample_in_kernel=True, edge_gate=gate),
                 lambda: a.fuse_views(rt, cams, probs, edge_gate=gate, view_weights=spec),        # view weights still need triangles
                 lambda: a.fuse_view_labels(r, cams[0], probs[0][:, :, 0].astype(np.uint8), edge_stats=True),
                 lambda: a.fuse_views_labels(r, cams, [p[:, :, 0].astype(np.uint8) for p in probs], edge_gate=3),
                 lambda: sm.fusion.edge_weights_device(sc["depth"][2], (3, 0.1)),
                 lambda: sm.fusion.edge_weights_device(sc["depth"][2], gate, np.ones((3, 3), np.float32))):
        with pytest.raises(ValueError):
            call()
        assert len(a._pending) == 1
    # the C entry points
    lib = sm._lib.lib()
    W, H = cams[0].resolution
    d_probs, d_sensor, d_depth = to_device(sc["probs"][2]), to_device(sc["sensors"][2]), to_device(sc["depth"][2])
    out = to_device(np.zeros((W, H), np.float32))
    pods = (sm._lib.CameraPOD * 1)(cams[0]._pod)
    iptr, sptr = (ctypes.c_void_p * 1)(d_probs.ptr), (ctypes.c_void_p * 1)(d_sensor.ptr)
    handle = a._handle
    nan, inf = float("nan"), float("inf")
    good = (3, 0.1, 0.0, 1, 0, 0)
    gpod = sm._lib.DepthGatePOD(0.001, 0.02, 0.0, inf, 1)
    vgood = (2, 0.3, 0, inf, inf)
    dummy = (ctypes.c_uint64 * 4)()

    def fuse(rh=r._h, edge=good, view=None, kind=sm._lib.PROBS_F32, sensors=None, dg_=None, w=W, h=H, vc=None, ec=None, dc=None, images=iptr):
        epod = None if edge is None else sm._lib.EdgeGatePOD(*edge)
        vpod = None if view is None else sm._lib.ViewWeightsPOD(*view)
        return lib.smesh_fuse_views_weighted(rh, handle, pods, 1, images, kind, None, None if vpod is None else ctypes.byref(vpod),
                                             None if epod is None else ctypes.byref(epod), sensors, sm._lib.DEPTH_U16, None, sm._lib.MEM_DEVICE, w, h,
                                             None if dg_ is None else ctypes.byref(dg_), vc, ec, dc)

    def single(edge=good, w=W, h=H, depth=d_depth.ptr, dst=out.ptr):
        epod = None if edge is None else sm._lib.EdgeGatePOD(*edge)
        return lib.smesh_edge_weights(ctypes.c_void_p(depth), w, h, None if epod is None else ctypes.byref(epod), None, ctypes.c_void_p(dst), None, 0)

    bad_gates = [(0, 0.1, 0.0, 1, 0, 0), (9, 0.1, 0.0, 1, 0, 0), (-3, 0.1, 0.0, 1, 0, 0), (3, nan, 0.0, 1, 0, 0), (3, -0.1, 0.0, 1, 0, 0),
                 (3, 0.1, nan, 1, 0, 0), (3, 0.1, -1.0, 1, 0, 0), (3, 0.1, 0.0, 2, 0, 0), (3, 0.1, 0.0, 1, -1, 0), (3, 0.1, 0.0, 1, 0, 7)]
    for kw in ([dict(edge=e) for e in bad_gates] +
               [dict(edge=None),                                                   # no stage at all
                dict(kind=5), dict(kind=-1), dict(images=None),
                dict(sensors=sptr), dict(dg_=gpod),                               # sensors and a depth gate go together
                dict(vc=dummy), dict(dc=dummy), dict(edge=None, view=vgood, ec=dummy),    # counts of a stage that is not given
                dict(view=(17, 0.3, 0, inf, inf)), dict(view=(2, nan, 0, inf, inf)), dict(view=(2, 0.3, 0, inf, 0.0)),
                dict(rh=rt._h, view=vgood),                                       # view weights need a triangle renderer
                dict(sensors=sptr, dg_=gpod, w=0), dict(sensors=sptr, dg_=gpod, h=65537),
                dict(sensors=sptr, dg_=sm._lib.DepthGatePOD(nan, 0.02, 0.0, inf, 1)), dict(sensors=sptr, dg_=sm._lib.DepthGatePOD(0.001, -1.0, 0.0, inf, 1))]):
        assert fuse(**kw) == sm._lib.ERR_INVALID, kw
        assert lib.smesh_last_error()
    for kw in [dict(edge=e) for e in bad_gates] + [dict(edge=None), dict(w=65537), dict(h=65537), dict(w=65536, h=8192), dict(depth=None), dict(dst=None)]:
        assert single(**kw) == sm._lib.ERR_INVALID, kw
    sm._lib.check(lib.smesh_synchronize(0))
    assert not out.numpy().any()
    assert option(sm, "edge_weights_launches") == launches
    assert len(a._pending) == 1
    with a._pending_lock:
        a._pending = []          # drop the deferred view: what is left must be the bits from before the refused calls
    np.testing.assert_array_equal(bits(a.get_raw()), before)
    sm._lib.check(lib.smesh_synchronize(0))


# ---- the effect ------------------------------------------------------------------------------------------------------------------
def test_the_gate_stops_labels_bleeding_across_an_occlusion_edge(sm):
    """A wall that fills the image and a smaller, nearer rectangle at least r + 1 pixels from every border, seen head-on.  The label
    image says 1 where the render shows the rectangle -- shifted by s = 3 pixels along y, as a pose error would, the vacated pixels
    0.  By construction (no code of the restatement): a wall pixel labelled 1 has a rectangle pixel 3 rows away in its column,
    inside its window of radius 3, one unit of depth nearer, far above t = 0.1 -- `behind` drops it; a rectangle pixel labelled 0 has
    a wall pixel 3 rows away -- `front` drops it.  Without the gate the wrong label reaches the wall."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.data import Camera, Mesh
    W, H, r, s = 160, 120, 3, 3
    wall = synth.grid_mesh(40, 40, extent=4.0, relief=0.0)
    rect = synth.grid_mesh(10, 8, extent=0.5, relief=0.0)          # 0.5 x 0.4, one unit in front of the wall
    wv, wf = np.asarray(wall.vertices, np.float32), np.asarray(wall.faces, np.int32)
    rv, rf = np.asarray(rect.vertices, np.float32) + np.float32([0, 0, 1]), np.asarray(rect.faces, np.int32)
    mesh = Mesh(np.concatenate([wv, rv]), np.concatenate([wf, rf + len(wv)]).astype(np.int32))
    Fw, P = len(wf), len(wf) + len(rf)
    R, tr = synth.look_at((0.0, 0.0, 6.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    cam = Camera(R, tr, np.asarray([W, H]), np.asarray([5.0 * W, 5.0 * W], np.float64), np.asarray([W / 2.0, H / 2.0], np.float64))
    rd = sm.render.triangles(mesh)
    idx, depth = (np.array(p) for p in rd.render(cam))
    assert np.isfinite(depth).all()                                 # the wall fills the image
    is_rect = idx >= Fw
    xs, ys = np.nonzero(is_rect)
    assert is_rect.sum() > 1000 and xs.min() >= r + 1 and ys.min() >= r + 1 and xs.max() <= W - 2 - r and ys.max() <= H - 2 - r
    assert depth[is_rect].max() < 5.1 and depth[~is_rect].min() > 5.9            # a step of one unit
    label = np.zeros((W, H), np.uint8)
    label[:, s:] = is_rect[:, :-s]
    bled = (label == 1) & ~is_rect
    assert bled.sum() > 100 and ((label == 0) & is_rect).sum() > 100

    def fused(**kw):
        a = sm.fusion.MeshAggregator(P, 2)
        a.fuse_views_labels(rd, [cam], [label], **kw)
        return a.get_raw()

    plain = fused()
    assert (plain[:Fw, 1] > 0).sum() > 0                            # without a gate the rectangle's label is on wall faces
    assert (plain[Fw:, 0] > 0).sum() > 0                            # and the wall's on the rectangle's rim
    behind = fused(edge_gate=sm.fusion.EdgeGate(r, 0.1, behind=True))
    assert not behind[:Fw, 1].any() and behind[:Fw, 0].sum() > 0 and behind[Fw:, 1].sum() > 0
    both = fused(edge_gate=sm.fusion.EdgeGate(r, 0.1, behind=True, front=True))
    assert not both[:Fw, 1].any() and not both[Fw:, 0].any()
    assert both[:Fw, 0].sum() > 0 and both[Fw:, 1].sum() > 0        # and what is away from the edge is still fused
