"""Fusion gated by sensor depth on the GPU (include/smesh_depth.h): `depth_weights` against depth_gate_ref in bytes, weights and counts;
the occluder scene, where the gate must reject a real share of every view; the gated fuse calls against the plain call and the CPU
oracle fed the restatement's weights -- bit for bit where one lane owns a row --; the per-view routes, the order of additions, the
all-consistent sensor, and the refusals."""
import ctypes

import numpy as np
import pytest

import depth_gate_ref as dg
from helpers import assert_fused_close, random_probs, small_scene
from test_gpu_label_prep import bits, layouts, option

pytestmark = pytest.mark.gpu

SHAPES = (((16, 12), (67, 45)), ((67, 45), (67, 45)), ((160, 120), (40, 30)), ((1, 1), (5, 3)))
C = 19
_cache = {}


def rendered_depth(sm, size):
    """The depth plane of a real render() of small_scene() at `size`, background included; rendered once per size."""
    if ("depth", size) not in _cache:
        mesh, cams = small_scene(width=size[0], height=size[1])
        depth = np.asarray(sm.render.triangles(mesh).render(cams[0])[1])
        assert depth.dtype == np.float32 and depth.shape == size
        assert np.isinf(depth).any() and np.isfinite(depth).any()
        _cache[("depth", size)] = depth
    return _cache[("depth", size)]


def make_sensor(rng, depth, shape, dtype):
    """A (w,h) sensor image around the scene's depths: most samples within a few centimetres of the rendered depth they meet, the
    rest off by up to a metre; zeros in a uint16 image, NaN, inf, 0 and negatives in a float32 one."""
    w, h = shape
    W, H = depth.shape
    near = depth[dg.axis_index(W, w)[:, None], dg.axis_index(H, h)[None, :]].astype(np.float64)
    near = np.where(np.isfinite(near), near, 7.0)
    noise = np.where(rng.random(shape) < 0.6, rng.uniform(-0.03, 0.03, shape), rng.uniform(-1.0, 1.0, shape))
    d = near + noise
    bad = rng.random(shape) < (0.1 if w * h > 1 else 0.0)
    if dtype == np.uint16:
        out = np.rint(1000.0 * d).astype(np.uint16)
        out[bad] = 0
        return out
    out = d.astype(np.float32)
    out[bad] = rng.choice(np.array([np.nan, np.inf, 0.0, -1.0, -np.inf], np.float32), size=int(bad.sum()))
    return out


def edge_plane(depth, sensor, g):
    """A second depth plane with hand-placed values: every pixel sits on the edge of its own tolerance, d_s + t or d_s - t, or one
    ulp to either side of it; the render's background stays background."""
    W, H = depth.shape
    raw = dg.sample(sensor, W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        d_s = raw.astype(np.float32) * g.scale
        t = g.abs_tol + g.rel_tol * d_s
        x, y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
        c = np.where((x + y) % 2 == 0, d_s + t, d_s - t).astype(np.float32)
        step = (x + 2 * y) % 3
        c = np.where(step == 1, np.nextafter(c, np.float32(np.inf)), np.where(step == 2, np.nextafter(c, np.float32(-np.inf)), c)).astype(np.float32)
    return np.where(np.isfinite(depth), c, depth).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_depth_weights_equal_the_restatement(sm, shape, dtype):
    """Every layout and memory of the sensor image, with and without weights_in, both missing policies, with and without max_depth:
    the bytes of depth_gate_ref.weights and its counts, on the render's plane and on the plane of edge values."""
    from semantic_meshes_amd.device import to_device
    (w, h), size = shape
    rng = np.random.default_rng(100 * w + h + (7 if dtype == np.float32 else 0))
    depth = rendered_depth(sm, size)
    sensor = make_sensor(rng, depth, (w, h), dtype)
    if w * h > 1:
        assert dg.missing_samples(sensor).any()
    w_in = rng.uniform(0.1, 2.0, size=size).astype(np.float32)
    d_depth, d_w_in = to_device(depth), to_device(w_in)
    seen = np.zeros(4, np.uint64)
    calls, edge_kept, edge_rejected = 0, 0, 0
    for missing in ("keep", "drop"):
        for max_depth in (None, 6.5):
            gate = sm.fusion.DepthGate(0.05, 0.004, None, max_depth, missing)
            g = dg.gate(0.05, 0.004, None, max_depth, missing, dtype)
            for weights in (None, w_in):
                want, want_counts = dg.weights(depth, sensor, g, weights)
                seen += want_counts
                for device in (False, True):
                    for layout, image in layouts(sensor, device).items():
                        before = option(sm, "depth_weights_launches")
                        got, counts = sm.fusion.depth_weights(d_depth, image, gate, None if weights is None else d_w_in, return_counts=True)
                        assert option(sm, "depth_weights_launches") - before == 1
                        calls += 1
                        msg = "%s device=%s missing=%s max_depth=%s weights=%s" % (layout, device, missing, max_depth, weights is not None)
                        np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)
                        np.testing.assert_array_equal(counts, want_counts, err_msg=msg)
            # the plane of edge values, the host forms of the depth plane and the weights, no counts
            edges = edge_plane(depth, sensor, g)
            want, want_counts = dg.weights(edges, sensor, g, w_in)
            kept = np.isfinite(edges) & (want != 0) & ~dg.missing_samples(dg.sample(sensor, *size))
            edge_kept, edge_rejected = edge_kept + int(kept.sum()), edge_rejected + int(want_counts[dg.INCONSISTENT])
            got = sm.fusion.depth_weights(edges, sensor, gate, w_in)
            np.testing.assert_array_equal(bits(got), bits(want))
            got, counts = sm.fusion.depth_weights(to_device(edges), to_device(sensor), gate, d_w_in, return_counts=True)
            np.testing.assert_array_equal(bits(got), bits(want))
            np.testing.assert_array_equal(counts, want_counts)
    print("    %d calls, counts %s, edge pixels kept %d rejected %d" % (calls, seen, edge_kept, edge_rejected))
    assert seen[dg.VISIBLE] > 0
    if size[0] * size[1] >= 1000:
        assert seen[dg.FAR] > 0 and seen[dg.INCONSISTENT] > 0 and edge_kept > 0 and edge_rejected > 0
        if w * h > 1:
            assert seen[dg.MISSING] > 0


def test_depth_weights_forms(sm):
    """A lazy render() plane as it comes, the result as the weights image of add(), and a depth plane that is not 16-byte aligned
    (the kernel's one-by-one form)."""
    from semantic_meshes_amd.device import to_device
    mesh, cams = small_scene()
    cam = cams[1]
    r = sm.render.triangles(mesh)
    depth = np.asarray(r.render(cam)[1])
    rng = np.random.default_rng(3)
    sensor = make_sensor(rng, depth, (80, 60), np.uint16)
    gate, g = sm.fusion.DepthGate(0.05, missing="drop"), dg.gate(0.05, missing="drop")
    want, _ = dg.weights(depth, sensor, g)
    assert (want == 0)[np.isfinite(depth)].any() and (want == 1).any()
    idx, d = r.render(cam)
    w = sm.fusion.depth_weights_device(d, np.ascontiguousarray(sensor.T).T, gate)
    assert w.shape == (160, 120) and w.dtype == np.float32
    np.testing.assert_array_equal(bits(w.numpy()), bits(want))
    probs = random_probs(rng, 160, 120, C)
    a, b = sm.fusion.MeshAggregator(len(mesh.faces), C), sm.fusion.MeshAggregator(len(mesh.faces), C)
    a.add(idx, probs, w)
    b.add(np.asarray(idx), probs, want)
    assert bits(b.get_raw()).any()
    assert_fused_close(a.get(), b.get())
    # a plane that starts four bytes behind a 16-byte boundary
    flat = to_device(np.concatenate([np.zeros(1, np.float32), depth.reshape(-1)]))
    from semantic_meshes_amd.device import DeviceArray
    off = DeviceArray(flat.ptr + 4, (160, 120), np.float32, flat.device, owner=flat)
    np.testing.assert_array_equal(bits(sm.fusion.depth_weights(off, sensor, gate)), bits(want))


# ---- the occluder scene ----------------------------------------------------------------------------------------------------------
def occluder(sm, oracle, size):
    """depth_gate_ref.occluder_scene with a product renderer, the render's own depth planes (equal to the oracle's in bits), class
    vectors and the restatement's weights; built once per size and left unchanged."""
    if ("occluder", size) not in _cache:
        mesh, cams, oidx, odepth, sensors, covered = dg.occluder_scene(oracle, *size)
        r = sm.render.triangles(mesh)
        queued = 0
        for k, cam in enumerate(cams):
            idx, depth = r.render(cam)
            np.testing.assert_array_equal(np.asarray(idx), oidx[k])
            np.testing.assert_array_equal(bits(np.asarray(depth)), bits(odepth[k]))
            queued += int(r.render_stats(cam, queues=True)[1][0])
        rng = np.random.default_rng(size[0])
        probs = [np.maximum(random_probs(rng, *size, C), 1e-3).astype(np.float32) for _ in cams]
        _cache[("occluder", size)] = dict(mesh=mesh, cams=cams, oidx=oidx, depth=odepth, sensors=sensors, probs=probs, P=len(mesh.faces),
                                          exact=queued == 0)
        print("    %s: %d queued triangles over the nine views" % (size, queued))
    return _cache[("occluder", size)]


def ref_weights(sc, g, weights_in=None, sensors=None):
    out = [dg.weights(sc["depth"][k], (sensors or sc["sensors"])[k], g, None if weights_in is None else weights_in[k]) for k in range(len(sc["cams"]))]
    return [w for w, _ in out], np.stack([c for _, c in out])


@pytest.mark.parametrize("size", dg.OCCLUDER_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_gate_rejects_what_the_occluder_covers(sm, oracle, size):
    """The stats of the gated fuse_views: in every view between 5 % and 95 % of the visible pixels are inconsistent, none missing,
    none far; with max_depth = 9 some view has far pixels and none has only far pixels.  A gate that passes or rejects everything
    fails here."""
    sc = occluder(sm, oracle, size)
    r = sm.render.triangles(sc["mesh"])
    agg = sm.fusion.MeshAggregator(sc["P"], C)
    stats = agg.fuse_views(r, sc["cams"], sc["probs"], sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02), depth_stats=True)
    assert stats.shape == (9, 4) and stats.dtype == np.uint64
    print("    inconsistent / visible: %s" % np.round(stats[:, 3] / stats[:, 0], 3))
    np.testing.assert_array_equal(stats, ref_weights(sc, dg.gate(0.02))[1])
    for v in range(9):
        assert 0.05 * stats[v, 0] <= stats[v, 3] <= 0.95 * stats[v, 0], stats[v]
        assert stats[v, 1] == 0 and stats[v, 2] == 0
    far = agg.fuse_views(r, sc["cams"], sc["probs"], sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02, max_depth=9.0), depth_stats=True)
    assert (far[:, 1] > 0).any() and (far[:, 1] < far[:, 0]).all()
    np.testing.assert_array_equal(far, ref_weights(sc, dg.gate(0.02, max_depth=9.0))[1])


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
def compare(sc, kind, got, plain, oagg_fill, oracle):
    """(i) against (ii) and (iii): bits for Sum / Summax where one lane owns every row, else the project's 1e-5."""
    if kind != "mul" and sc["exact"]:
        oagg = oagg_fill()
        assert bits(oagg.get_raw()).any()
        np.testing.assert_array_equal(bits(got.get_raw()), bits(plain.get_raw()))
        np.testing.assert_array_equal(bits(got.get_raw()), bits(oagg.get_raw()))
        np.testing.assert_array_equal(bits(got.get()), bits(oagg.get()))
        return
    oracle.set_accum_double(True)
    try:
        want = oagg_fill().get()
    finally:
        oracle.set_accum_double(False)
    assert np.abs(want).sum() > 0
    assert_fused_close(got.get(), plain.get())
    assert_fused_close(got.get(), want)


@pytest.mark.parametrize("kind", ["sum", "summax", "mul"])
@pytest.mark.parametrize("size", dg.OCCLUDER_SIZES, ids=lambda s: "%dx%d" % s)
def test_gated_fuse_views_is_the_plain_call_with_the_rules_weights(sm, oracle, size, kind):
    """Nine views -- a group of eight and a remainder -- with device class vectors: (i) the gated call, (ii) fuse_views with the
    restatement's weights images, (iii) the oracle's add() with the same; the same kernel, one k_depth_weights launch per group."""
    from semantic_meshes_amd.device import to_device
    sc = occluder(sm, oracle, size)
    if size == (96, 64):
        assert sc["exact"]      # (no queued triangle at this size: the bit-for-bit leg really runs)
    r = sm.render.triangles(sc["mesh"])
    Wref, counts = ref_weights(sc, dg.gate(0.02))
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C, kind)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wref])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C, kind)
    before = option(sm, "depth_weights_launches")
    stats = got.fuse_views(r, sc["cams"], d_probs, sensor_depths=[to_device(s) for s in sc["sensors"]], depth_gate=sm.fusion.DepthGate(0.02),
                           depth_stats=True)
    assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith("k_fuse_tri")
    assert option(sm, "depth_weights_launches") - before == 2
    np.testing.assert_array_equal(stats, counts)

    def fill():
        oagg = oracle.OracleAggregator(sc["P"], C, kind)
        for k in range(9):
            oagg.add(sc["oidx"][k], sc["probs"][k], Wref[k])
        return oagg
    compare(sc, kind, got, plain, fill, oracle)
    # without the stats the call does the same
    again = sm.fusion.MeshAggregator(sc["P"], C, kind)
    assert again.fuse_views(r, sc["cams"], sc["probs"], sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02)) is None
    compare(sc, kind, again, plain, fill, oracle)


def test_gated_forms(sm, oracle):
    """float16 images, a uint8 mask through fuse_views_labels, a caller's weights multiplied in, a sensor at half the camera's size
    (as the transposed view of the decoded image), a mask at half the size through a map: each against the plain call with the
    restatement's weights, in bits, with the plain call's kernel."""
    from semantic_meshes_amd.device import to_device
    size = (96, 64)
    sc = occluder(sm, oracle, size)
    assert sc["exact"]
    r = sm.render.triangles(sc["mesh"])
    gate, g = sm.fusion.DepthGate(0.02), dg.gate(0.02)
    Wref, _ = ref_weights(sc, g)
    rng = np.random.default_rng(11)

    def twin(gated, plain, kernel_prefix):
        a, b = sm.fusion.MeshAggregator(sc["P"], C), sm.fusion.MeshAggregator(sc["P"], C)
        plain(b)
        kernel = sm._lib.last_fuse_kernel()
        gated(a)
        assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith(kernel_prefix), kernel
        assert bits(b.get_raw()).any()
        np.testing.assert_array_equal(bits(a.get_raw()), bits(b.get_raw()))

    # float16 class vectors
    half = [sm.fusion.narrow_probs(p, "float16") for p in sc["probs"]]
    twin(lambda a: a.fuse_views(r, sc["cams"], half, sensor_depths=sc["sensors"], depth_gate=gate),
         lambda b: b.fuse_views(r, sc["cams"], half, [to_device(w) for w in Wref]), "k_fuse_tri_h16")
    # a uint8 mask
    masks = [rng.integers(0, C + 2, size=size).astype(np.uint8) for _ in sc["cams"]]
    twin(lambda a: a.fuse_views_labels(r, sc["cams"], masks, sensor_depths=sc["sensors"], depth_gate=gate),
         lambda b: b.fuse_views_labels(r, sc["cams"], masks, Wref), "k_fuse_tri_labels")
    # a mask at half the size and in other ids
    small = [rng.integers(0, 40, size=(48, 32)).astype(np.int32) for _ in sc["cams"]]
    table = rng.integers(-1, C, size=40).astype(np.int32)
    twin(lambda a: a.fuse_views_labels(r, sc["cams"], small, resize="nearest", label_map=table, sensor_depths=sc["sensors"], depth_gate=gate),
         lambda b: b.fuse_views_labels(r, sc["cams"], small, Wref, resize="nearest", label_map=table), "k_fuse_tri_labels")
    # the caller's weights are multiplied in (host arrays)
    mine = [rng.uniform(0.1, 2.0, size=size).astype(np.float32) for _ in sc["cams"]]
    Wmul, _ = ref_weights(sc, g, mine)
    assert any((w != v).any() for w, v in zip(Wmul, Wref))
    twin(lambda a: a.fuse_views(r, sc["cams"], sc["probs"], mine, sensor_depths=sc["sensors"], depth_gate=gate),
         lambda b: b.fuse_views(r, sc["cams"], [to_device(p) for p in sc["probs"]], [to_device(w) for w in Wmul]), "k_fuse_tri")
    # a sensor at half the camera's size, decoded as (h,w)
    halves = [np.ascontiguousarray(s[::2, ::2].T) for s in sc["sensors"]]
    loose, gl = sm.fusion.DepthGate(0.05), dg.gate(0.05)
    Whalf, chalf = ref_weights(sc, gl, sensors=[x.T for x in halves])
    assert all(0 < c[3] < c[0] for c in chalf)
    twin(lambda a: a.fuse_views(r, sc["cams"], sc["probs"], sensor_depths=[x.T for x in halves], depth_gate=loose),
         lambda b: b.fuse_views(r, sc["cams"], [to_device(p) for p in sc["probs"]], [to_device(w) for w in Whalf]), "k_fuse_tri")
    # resize="bilinear": resampled, then gated
    tiny = [np.ascontiguousarray(p[::2, ::2]) for p in sc["probs"]]
    twin(lambda a: a.fuse_views(r, sc["cams"], tiny, resize="bilinear", sensor_depths=sc["sensors"], depth_gate=gate),
         lambda b: b.fuse_views(r, sc["cams"], tiny, [to_device(w) for w in Wref], resize="bilinear"), "k_fuse_tri")


def test_the_per_view_route(sm, oracle):
    """A texel renderer, and an aggregator of 200 classes: no eight-view launch of the k_fuse_tri family serves them, the views are
    fused one by one from the same weights planes -- the plain call with the restatement's weights within the project's 1e-5, the
    200 classes also against the float64 oracle."""
    from semantic_meshes_amd.device import to_device
    size = (96, 64)
    sc = occluder(sm, oracle, size)
    gate, g = sm.fusion.DepthGate(0.02), dg.gate(0.02)
    Wref, counts = ref_weights(sc, g)
    rt = sm.render.texels(sc["mesh"], sc["cams"], 0.05)
    a, b = sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C), sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C)
    before = option(sm, "depth_weights_launches")
    stats = a.fuse_views(rt, sc["cams"], sc["probs"], sensor_depths=sc["sensors"], depth_gate=gate, depth_stats=True)
    assert option(sm, "depth_weights_launches") - before == 2
    assert sm._lib.last_fuse_kernel() == "k_fuse_texel"
    np.testing.assert_array_equal(stats, counts)
    b.fuse_views(rt, sc["cams"], [to_device(p) for p in sc["probs"]], [to_device(w) for w in Wref])
    assert np.abs(b.get()).sum() > 0
    assert_fused_close(a.get(), b.get())
    # 200 classes
    wide = 200
    rng = np.random.default_rng(5)
    probs = [random_probs(rng, *size, wide) for _ in sc["cams"]]
    r = sm.render.triangles(sc["mesh"])
    a, b = sm.fusion.MeshAggregator(sc["P"], wide), sm.fusion.MeshAggregator(sc["P"], wide)
    a.fuse_views(r, sc["cams"], probs, sensor_depths=sc["sensors"], depth_gate=gate)
    kernel = sm._lib.last_fuse_kernel()
    b.fuse_views(r, sc["cams"], [to_device(p) for p in probs], [to_device(w) for w in Wref])
    assert sm._lib.last_fuse_kernel() == kernel
    assert_fused_close(a.get(), b.get())
    oracle.set_accum_double(True)
    try:
        oagg = oracle.OracleAggregator(sc["P"], wide)
        for k in range(9):
            oagg.add(sc["oidx"][k], probs[k], Wref[k])
        want = oagg.get()
    finally:
        oracle.set_accum_double(False)
    assert_fused_close(a.get(), want)


def test_a_gated_fuse_view_keeps_the_order_of_additions(sm, oracle):
    """Two deferred views, then a gated fuse_view (and a gated fuse_view_labels): the deferred views are handed over first -- the
    bits of the same sequence issued eagerly, and of the oracle."""
    from semantic_meshes_amd.device import to_device
    from test_labels_host import one_hot
    size = (96, 64)
    sc = occluder(sm, oracle, size)
    assert sc["exact"]
    r = sm.render.triangles(sc["mesh"])
    gate, g = sm.fusion.DepthGate(0.02), dg.gate(0.02)
    Wref, counts = ref_weights(sc, g)
    mask = np.random.default_rng(2).integers(0, C, size=size).astype(np.uint8)
    got = []
    for defer in (True, False):
        a = sm.fusion.MeshAggregator(sc["P"], C, "sum", 0.5)
        a.defer = defer
        a.fuse_view(r, sc["cams"][0], to_device(sc["probs"][0]))
        a.fuse_view(r, sc["cams"][1], to_device(sc["probs"][1]))
        assert len(a._pending) == (2 if defer else 0)
        stats = a.fuse_view(r, sc["cams"][2], sc["probs"][2], sensor_depth=sc["sensors"][2], depth_gate=gate, depth_stats=True)
        assert len(a._pending) == 0
        np.testing.assert_array_equal(stats, counts[2])
        a.fuse_view(r, sc["cams"][3], to_device(sc["probs"][3]))
        assert a.fuse_view_labels(r, sc["cams"][4], mask, sensor_depth=to_device(sc["sensors"][4]), depth_gate=gate) is None
        assert len(a._pending) == 0
        got.append(bits(a.get_raw()))
    np.testing.assert_array_equal(got[0], got[1])
    oagg = oracle.OracleAggregator(sc["P"], C, "sum", 0.5)
    for k in range(4):
        oagg.add(sc["oidx"][k], sc["probs"][k], Wref[k] if k == 2 else None)
    oagg.add(sc["oidx"][4], one_hot(mask, C), Wref[4])
    np.testing.assert_array_equal(got[0], bits(oagg.get_raw()))


def test_an_all_consistent_sensor_changes_nothing(sm, oracle):
    """A sensor that agrees with the render everywhere (the render's own depth as float32, and as millimetres within 2 cm): the gated
    call is the plain call, in bits."""
    from semantic_meshes_amd.device import to_device
    size = (96, 64)
    sc = occluder(sm, oracle, size)
    assert sc["exact"]
    r = sm.render.triangles(sc["mesh"])
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C, "summax")
    plain.fuse_views(r, sc["cams"], d_probs)
    kernel = sm._lib.last_fuse_kernel()
    exact = [np.where(np.isfinite(d), d, np.float32(0)) for d in sc["depth"]]
    millimetres = [np.rint(1000.0 * x.astype(np.float64)).astype(np.uint16) for x in exact]
    for sensors, gate in ((exact, sm.fusion.DepthGate(0.0, missing="drop")), (millimetres, sm.fusion.DepthGate(0.02, missing="drop"))):
        a = sm.fusion.MeshAggregator(sc["P"], C, "summax")
        stats = a.fuse_views(r, sc["cams"], d_probs, sensor_depths=sensors, depth_gate=gate, depth_stats=True)
        assert sm._lib.last_fuse_kernel() == kernel
        assert (stats[:, 0] > 0).all() and not stats[:, 1:].any()
        np.testing.assert_array_equal(bits(a.get_raw()), bits(plain.get_raw()))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(sm, oracle):
    from semantic_meshes_amd.device import to_device
    size = (96, 64)
    sc = occluder(sm, oracle, size)
    r = sm.render.triangles(sc["mesh"])
    gate = sm.fusion.DepthGate(0.02)
    a = sm.fusion.MeshAggregator(sc["P"], C)
    a.fuse_view(r, sc["cams"][0], sc["probs"][0], sensor_depth=sc["sensors"][0], depth_gate=gate)
    before = bits(a.get_raw()).copy()
    assert before.any()
    a.fuse_view(r, sc["cams"][1], to_device(sc["probs"][1]))       # one deferred view: a refused call must leave it pending
    assert len(a._pending) == 1
    cams, probs, sensors = sc["cams"][2:4], sc["probs"][2:4], sc["sensors"][2:4]
    for call in (lambda: a.fuse_views(r, cams, probs, sensor_depths=sensors), lambda: a.fuse_views(r, cams, probs, depth_gate=gate),
                 lambda: a.fuse_views(r, cams, probs, sensor_depths=sensors[:1], depth_gate=gate),
                 lambda: a.fuse_views(r, cams, probs, sensor_depths=[sensors[0], sensors[1].astype(np.int16)], depth_gate=gate),
                 lambda: a.fuse_views(r, cams, probs, resize="bilinear", sample_in_kernel=True, sensor_depths=sensors, depth_gate=gate),
                 lambda: a.fuse_view_labels(r, cams[0], probs[0][:, :, 0].astype(np.uint8), sensor_depth=sensors[0])):
        with pytest.raises(ValueError):
            call()
        assert len(a._pending) == 1
    # the C entry point
    lib = sm._lib.lib()
    d_probs, d_sensor = to_device(sc["probs"][2]), to_device(sc["sensors"][2])
    pods = (sm._lib.CameraPOD * 1)(sc["cams"][2]._pod)
    iptr, sptr = (ctypes.c_void_p * 1)(d_probs.ptr), (ctypes.c_void_p * 1)(d_sensor.ptr)
    handle = a._handle
    nan = float("nan")

    def fuse(kind=sm._lib.PROBS_F32, dtype=sm._lib.DEPTH_U16, strides=None, mem=sm._lib.MEM_DEVICE, w=size[0], h=size[1], gate_values=(0.001, 0.02, 0.0, np.inf, 1)):
        pod = sm._lib.DepthGatePOD(*gate_values)
        return lib.smesh_fuse_views_depth(r._h, handle, pods, 1, iptr, kind, None, sptr, dtype, strides, mem, w, h, ctypes.byref(pod), None)

    for kw in (dict(w=0), dict(h=0), dict(w=65537), dict(h=65537), dict(strides=(ctypes.c_int64 * 2)(-1, 1)), dict(strides=(ctypes.c_int64 * 2)(64, -1)),
               dict(dtype=2), dict(dtype=-1), dict(mem=2), dict(kind=5), dict(kind=-1), dict(gate_values=(nan, 0.02, 0.0, np.inf, 1)),
               dict(gate_values=(-1.0, 0.02, 0.0, np.inf, 1)), dict(gate_values=(0.001, nan, 0.0, np.inf, 1)), dict(gate_values=(0.001, -0.02, 0.0, np.inf, 1)),
               dict(gate_values=(0.001, 0.02, nan, np.inf, 1)), dict(gate_values=(0.001, 0.02, -0.5, np.inf, 1)), dict(gate_values=(0.001, 0.02, 0.0, nan, 1))):
        assert fuse(**kw) == sm._lib.ERR_INVALID, kw
        assert lib.smesh_last_error()
    pod = sm._lib.DepthGatePOD(0.001, 0.02, 0.0, np.inf, 1)
    assert lib.smesh_fuse_views_depth(r._h, handle, pods, 1, iptr, 0, None, sptr, 0, None, 1, size[0], size[1], None, None) == sm._lib.ERR_INVALID
    out = to_device(np.zeros(size, np.float32))
    d_depth = to_device(sc["depth"][2])
    for w, h, dtype, gv in ((0, 4, 0, (0.001, 0.02, 0.0, np.inf, 1)), (4, 4, 7, (0.001, 0.02, 0.0, np.inf, 1)), (4, 4, 0, (0.001, nan, 0.0, np.inf, 1))):
        pod = sm._lib.DepthGatePOD(*gv)
        assert lib.smesh_depth_weights(ctypes.c_void_p(d_depth.ptr), size[0], size[1], ctypes.c_void_p(d_sensor.ptr), dtype, None, 1, w, h, ctypes.byref(pod), None,
                                       ctypes.c_void_p(out.ptr), None, 0) == sm._lib.ERR_INVALID
    assert not out.numpy().any()
    assert len(a._pending) == 1
    with a._pending_lock:
        a._pending = []          # drop the deferred view: what is left must be the bits from before the refused calls
    np.testing.assert_array_equal(bits(a.get_raw()), before)
    sm._lib.check(lib.smesh_synchronize(0))
