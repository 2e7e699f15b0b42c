"""Fusion weighted by viewing geometry on the GPU (include/smesh_view_weights.h): `view_weights` against view_weights_ref in bits,
weights and counts, at the sizes where the kernel changes its path; a mesh processed in Morton order; the weighted fuse calls against
the plain call fed the restatement's planes -- bit for bit where one lane owns a row --; the label and 16-bit forms; the combination
with the depth gate; the per-view route and the order of additions; the identity spec; the refusals; and a floor seen frontally and
at 80 degrees, where the weights must decide the label."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_gate_ref as dg
import view_weights_ref as vw
from helpers import assert_fused_close, random_probs, small_scene
from test_gpu_label_prep import bits, option

pytestmark = pytest.mark.gpu

C = 19
SIZES = ((37, 29), (97, 61), (200, 180))      # N mod 4 != 0 and a partly empty chunk; two chunks; nine chunks
FUSE_SIZES = ((96, 64), (80, 56))             # two camera resolutions inside one group
VIEWS = 11                                    # a full group of eight plus three
_cache = {}


def rewound_mesh():
    """small_scene's mesh with every third face re-wound (it looks away from the cameras above it; the rasteriser does not cull) and
    one face made degenerate."""
    from semantic_meshes_amd.data import Mesh
    mesh, _ = small_scene()
    faces = np.array(mesh.faces, np.int32)
    faces[::3] = faces[::3, ::-1]
    faces[7] = (faces[7, 0], faces[7, 0], faces[7, 1])
    return Mesh(np.asarray(mesh.vertices, np.float32), faces)


def rendered(sm, size):
    """(mesh, camera, renderer, idx, depth, normals) of a real render() of the re-wound scene at `size`; rendered once per size."""
    if ("render", size) not in _cache:
        mesh = rewound_mesh()
        cam = small_scene(width=size[0], height=size[1])[1][1]
        r = sm.render.triangles(mesh)
        idx, depth = (np.asarray(p) for p in r.render(cam))
        assert idx.dtype == np.uint32 and depth.dtype == np.float32 and idx.shape == depth.shape == size
        assert np.isinf(depth).any() and np.isfinite(depth).any()
        _cache[("render", size)] = (mesh, cam, r, idx, depth, vw.face_normals(mesh.vertices, mesh.faces))
    return _cache[("render", size)]


SPECS = [(0, 0.0, True, None, None), (1, 0.0, True, None, None), (4, 0.3, True, None, None), (1, 0.3, False, None, None),
         (4, 0.0, False, 6.5, None), (1, 0.3, True, None, 3.0), (0, 0.3, False, 6.5, 3.0),
         (2, 0.8, True, None, None)]          # (no pixel of these views is seen below a cosine of 0.3: a cut-off that rejects some)


def check_kernel_against_restatement(sm, size):
    from semantic_meshes_amd.device import to_device
    mesh, cam, r, idx, depth, normals = rendered(sm, size)
    rng = np.random.default_rng(size[0])
    w_in = rng.uniform(0.1, 2.0, size=size).astype(np.float32)
    d_idx, d_depth, d_w = to_device(idx), to_device(depth), to_device(w_in)
    seen = np.zeros(4, np.uint64)
    for args in SPECS:
        spec, s = sm.fusion.ViewWeights(*args), vw.spec(*args)
        for weights, d_weights in ((None, None), (w_in, d_w)):
            want, want_counts = vw.weights(cam, normals, idx, depth, s, weights)
            seen += want_counts
            before = option(sm, "view_weights_launches")
            got, counts = sm.fusion.view_weights(r, cam, d_idx, d_depth, spec, d_weights, return_counts=True)
            assert option(sm, "view_weights_launches") - before == 1
            msg = "%s %s weights=%s" % (size, spec, weights is not None)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)
            np.testing.assert_array_equal(counts, want_counts, err_msg=msg)
        # host planes, no counts
        np.testing.assert_array_equal(bits(sm.fusion.view_weights(r, cam, idx, depth, spec, w_in)), bits(vw.weights(cam, normals, idx, depth, s, w_in)[0]))
    print("    %s: counts over the specs %s" % (size, seen))
    assert seen[vw.VISIBLE] > 0 and seen[vw.FAR] > 0 and seen[vw.GRAZING] > 0 and seen[vw.BACKFACING] > 0
    return mesh, cam, r, idx, depth, normals, w_in


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_view_weights_equal_the_restatement(sm, size):
    """With and without weights_image, two_sided 0 / 1, power 0 / 1 / 4, min_cos 0 / 0.3, with max_depth and falloff_depth: the bits
    of view_weights_ref.weights and its counts, one launch per call."""
    check_kernel_against_restatement(sm, size)


def test_view_weights_in_unaligned_planes(sm):
    """A weights-in plane, and a weights-out plane, four bytes behind a 16-byte boundary: the kernel's one-by-one form.  (The output
    of the Python layer is its own allocation, so the unaligned output goes through the C entry point.)"""
    from semantic_meshes_amd.device import DeviceArray, to_device
    size = (97, 61)
    mesh, cam, r, idx, depth, normals = rendered(sm, size)
    w_in = np.random.default_rng(9).uniform(0.1, 2.0, size=size).astype(np.float32)
    args = (4, 0.3, False, 6.5, 3.0)
    spec, s = sm.fusion.ViewWeights(*args), vw.spec(*args)
    want, want_counts = vw.weights(cam, normals, idx, depth, s, w_in)
    flat = to_device(np.concatenate([np.zeros(1, np.float32), w_in.reshape(-1)]))
    off = DeviceArray(flat.ptr + 4, size, np.float32, flat.device, owner=flat)
    assert off.ptr % 16 == 4
    got, counts = sm.fusion.view_weights(r, cam, to_device(idx), to_device(depth), spec, off, return_counts=True)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(counts, want_counts)
    out = to_device(np.full(size[0] * size[1] + 2, -1.0, np.float32))
    d_idx, d_depth, d_w = to_device(idx), to_device(depth), to_device(w_in)
    pod = spec._pod()
    sm._lib.check(sm._lib.lib().smesh_view_weights(r._h, ctypes.byref(cam._pod), ctypes.c_void_p(d_idx.ptr), ctypes.c_void_p(d_depth.ptr), size[0], size[1],
                                                   ctypes.byref(pod), ctypes.c_void_p(d_w.ptr), ctypes.c_void_p(out.ptr + 4), None))
    sm._lib.check(sm._lib.lib().smesh_synchronize(0))
    host = out.numpy()
    assert host[0] == -1.0 and host[-1] == -1.0                 # nothing written outside the plane
    np.testing.assert_array_equal(bits(host[1:-1].reshape(size)), bits(want))


def _child(test_name, **env):
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", test_name, "-p",
                          "no:cacheprovider"], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_reordered_mesh_child(sm):
    """SMESH_REORDER=1 (read when the renderer is made): the mesh is processed in Morton order behind a position -> id table; the
    normals table is indexed by what the index plane holds, the caller's face id -- the restatement's weights, and a weighted
    fuse_views equal to the plain call with them."""
    if os.environ.get("SMESH_REORDER") != "1":
        _child("test_reordered_mesh_child", SMESH_REORDER="1")
        return
    from semantic_meshes_amd.device import to_device
    mesh, cam, r, idx, depth, normals, w_in = check_kernel_against_restatement(sm, (97, 61))
    args = (2, 0.3, False, None, None)
    want = vw.weights(cam, normals, idx, depth, vw.spec(*args), w_in)[0]
    probs = random_probs(np.random.default_rng(4), 97, 61, C)
    a, b = sm.fusion.MeshAggregator(len(mesh.faces), C), sm.fusion.MeshAggregator(len(mesh.faces), C)
    a.fuse_views(r, [cam], [probs], [w_in], view_weights=sm.fusion.ViewWeights(*args))
    b.fuse_views(r, [cam], [to_device(probs)], [to_device(want)])
    assert np.abs(b.get()).sum() > 0
    assert_fused_close(a.get(), b.get())


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
def fuse_scene(sm):
    """Eleven ring cameras over the re-wound mesh, alternating between two resolutions, with the render's own planes, class vectors,
    caller's weights and uint16 sensor images of one size, a third of whose samples are off; built once and left unchanged."""
    if "fuse" not in _cache:
        from semantic_meshes_amd import synth
        mesh = rewound_mesh()
        cams = [synth.ring_camera(k, VIEWS, *FUSE_SIZES[k % 2]) for k in range(VIEWS)]
        r = sm.render.triangles(mesh)
        rng = np.random.default_rng(21)
        idx, depth, probs, mine, sensors, queued = [], [], [], [], [], 0
        for cam in cams:
            i, d = (np.array(p) for p in r.render(cam))
            queued += int(r.render_stats(cam, queues=True)[1][0])
            idx.append(i)
            depth.append(d)
            probs.append(np.maximum(random_probs(rng, *cam.resolution, C), 1e-3).astype(np.float32))
            mine.append(rng.uniform(0.1, 2.0, size=cam.resolution).astype(np.float32))
            # (one sensor size for all views, so that a chunk of eight is one library call: the render's depth sampled to it)
            near = d[dg.axis_index(d.shape[0], FUSE_SIZES[0][0])[:, None], dg.axis_index(d.shape[1], FUSE_SIZES[0][1])[None, :]].astype(np.float64)
            mm = np.where(np.isfinite(near), np.rint(1000.0 * near + np.where(rng.random(near.shape) < 0.3, 500.0, 0.0)), 0.0)
            sensors.append(mm.astype(np.uint16))
        _cache["fuse"] = dict(mesh=mesh, cams=cams, idx=idx, depth=depth, probs=probs, mine=mine, sensors=sensors, P=len(mesh.faces),
                              normals=vw.face_normals(mesh.vertices, mesh.faces), exact=queued == 0)
        print("    %d queued triangles over the eleven views" % queued)
    return _cache["fuse"]


def ref_planes(sc, s, weights_in=None):
    out = [vw.weights(sc["cams"][k], sc["normals"], sc["idx"][k], sc["depth"][k], s, None if weights_in is None else weights_in[k]) for k in range(VIEWS)]
    return [w for w, _ in out], np.stack([c for _, c in out])


def same(sc, kind, got, want):
    """Bits for Sum / Summax where one lane owns every row, else the project's 1e-5."""
    assert np.abs(want.get()).sum() > 0
    if kind != "mul" and sc["exact"]:
        np.testing.assert_array_equal(bits(got.get_raw()), bits(want.get_raw()))
    else:
        assert_fused_close(got.get(), want.get())


SPEC = (2, 0.3, False, 7.5, 4.0)


@pytest.mark.parametrize("kind", ["sum", "summax", "mul"])
def test_weighted_fuse_views_is_the_plain_call_with_the_rules_weights(sm, kind):
    """Eleven views -- a group of eight and a remainder, two resolutions inside a group -- with device class vectors and the caller's
    weights: the plain call with the restatement's planes; the same kernel, one k_view_weights launch per group, the counts."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    Wref, counts = ref_planes(sc, vw.spec(*SPEC), sc["mine"])
    assert (counts[:, 1:] > 0).any(axis=0).all() and all(0 < (w > 0).sum() for w in Wref)
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C, kind)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wref])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C, kind)
    before = option(sm, "view_weights_launches"), option(sm, "depth_weights_launches")
    stats = got.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in sc["mine"]], view_weights=sm.fusion.ViewWeights(*SPEC), view_stats=True)
    assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith("k_fuse_tri")
    assert option(sm, "view_weights_launches") - before[0] == 2 and option(sm, "depth_weights_launches") == before[1]
    assert stats.shape == (VIEWS, 4) and stats.dtype == np.uint64
    np.testing.assert_array_equal(stats, counts)
    same(sc, kind, got, plain)
    # host images, no stats: the same
    again = sm.fusion.MeshAggregator(sc["P"], C, kind)
    assert again.fuse_views(r, sc["cams"], sc["probs"], sc["mine"], view_weights=sm.fusion.ViewWeights(*SPEC)) is None
    same(sc, kind, again, plain)


def test_label_and_16_bit_forms(sm):
    """fuse_views_labels(view_weights=) and a float16 fuse_views: each the plain call with the restatement's planes, with its kernel."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    spec = sm.fusion.ViewWeights(*SPEC)
    Wref, _ = ref_planes(sc, vw.spec(*SPEC))
    rng = np.random.default_rng(13)

    def twin(weighted, plain, prefix):
        a, b = sm.fusion.MeshAggregator(sc["P"], C), sm.fusion.MeshAggregator(sc["P"], C)
        plain(b)
        kernel = sm._lib.last_fuse_kernel()
        weighted(a)
        assert sm._lib.last_fuse_kernel() == kernel and kernel.startswith(prefix), kernel
        same(sc, "sum", a, b)

    half = [sm.fusion.narrow_probs(p, "float16") for p in sc["probs"]]
    twin(lambda a: a.fuse_views(r, sc["cams"], half, view_weights=spec), lambda b: b.fuse_views(r, sc["cams"], half, [to_device(w) for w in Wref]),
         "k_fuse_tri_h16")
    masks = [rng.integers(0, C + 2, size=cam.resolution).astype(np.uint8) for cam in sc["cams"]]
    twin(lambda a: a.fuse_views_labels(r, sc["cams"], masks, view_weights=spec), lambda b: b.fuse_views_labels(r, sc["cams"], masks, Wref),
         "k_fuse_tri_labels")


def test_view_weights_then_depth_gate(sm):
    """Both keywords: the plain call with depth_gate_ref applied to the view-weights planes as its weights-in; both stats arrays;
    one launch of each kernel per group."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    Wview, vcounts = ref_planes(sc, vw.spec(*SPEC), sc["mine"])
    g = dg.gate(0.02, missing="drop")
    both = [dg.weights(sc["depth"][k], sc["sensors"][k], g, Wview[k]) for k in range(VIEWS)]
    Wref, dcounts = [w for w, _ in both], np.stack([c for _, c in both])
    assert all((a != b).any() for a, b in zip(Wref, Wview)) and (dcounts[:, dg.INCONSISTENT] > 0).all()
    np.testing.assert_array_equal(dcounts, np.stack([dg.weights(sc["depth"][k], sc["sensors"][k], g)[1] for k in range(VIEWS)]))   # a zero stays zero
    d_probs = [to_device(p) for p in sc["probs"]]
    plain = sm.fusion.MeshAggregator(sc["P"], C)
    plain.fuse_views(r, sc["cams"], d_probs, [to_device(w) for w in Wref])
    kernel = sm._lib.last_fuse_kernel()
    got = sm.fusion.MeshAggregator(sc["P"], C)
    before = option(sm, "view_weights_launches"), option(sm, "depth_weights_launches")
    stats = got.fuse_views(r, sc["cams"], d_probs, sc["mine"], sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02, missing="drop"),
                           depth_stats=True, view_weights=sm.fusion.ViewWeights(*SPEC), view_stats=True)
    assert sm._lib.last_fuse_kernel() == kernel
    assert option(sm, "view_weights_launches") - before[0] == 2 and option(sm, "depth_weights_launches") - before[1] == 2
    assert isinstance(stats, tuple) and len(stats) == 2
    np.testing.assert_array_equal(stats[0], vcounts)
    np.testing.assert_array_equal(stats[1], dcounts)
    same(sc, "sum", got, plain)
    # one stats consumer each
    a = sm.fusion.MeshAggregator(sc["P"], C)
    only = a.fuse_views(r, sc["cams"], d_probs, sc["mine"], sensor_depths=sc["sensors"], depth_gate=sm.fusion.DepthGate(0.02, missing="drop"),
                        depth_stats=True, view_weights=sm.fusion.ViewWeights(*SPEC))
    np.testing.assert_array_equal(only, dcounts)
    same(sc, "sum", a, plain)


def test_the_per_view_route_and_the_order_of_additions(sm):
    """render() + view_weights_device + add(idx, probs, w) per view: the sums of the weighted fuse_views.  Two deferred views, then a
    weighted fuse_view (and a weighted fuse_view_labels): the deferred views are handed over first -- the bits of the same sequence
    issued eagerly, and of the plain calls with the restatement's planes."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    spec = sm.fusion.ViewWeights(*SPEC)
    Wref, counts = ref_planes(sc, vw.spec(*SPEC))
    batch = sm.fusion.MeshAggregator(sc["P"], C)
    batch.fuse_views(r, sc["cams"], sc["probs"], view_weights=spec)
    each = sm.fusion.MeshAggregator(sc["P"], C)
    for k, cam in enumerate(sc["cams"]):
        idx, depth = r.render(cam)
        w, c = sm.fusion.view_weights_device(r, cam, idx, depth, spec, return_counts=True)
        assert w.shape == cam.resolution and w.dtype == np.float32
        np.testing.assert_array_equal(c, counts[k])
        np.testing.assert_array_equal(bits(w.numpy()), bits(Wref[k]))
        each.add(idx, to_device(sc["probs"][k]), w)
    same(sc, "sum", each, batch)
    # (views 0, 2, 4, 6, 8 share a resolution: a deferred group holds views of one size)
    v = [0, 2, 4, 6, 8]
    mask = np.random.default_rng(2).integers(0, C, size=sc["cams"][v[4]].resolution).astype(np.uint8)
    got, aggs = [], []
    for defer in (True, False):
        a = sm.fusion.MeshAggregator(sc["P"], C, "sum", 0.5)
        aggs.append(a)
        a.defer = defer
        a.fuse_view(r, sc["cams"][v[0]], to_device(sc["probs"][v[0]]))
        a.fuse_view(r, sc["cams"][v[1]], to_device(sc["probs"][v[1]]))
        assert len(a._pending) == (2 if defer else 0)
        stats = a.fuse_view(r, sc["cams"][v[2]], sc["probs"][v[2]], view_weights=spec, view_stats=True)
        assert len(a._pending) == 0
        np.testing.assert_array_equal(stats, counts[v[2]])
        a.fuse_view(r, sc["cams"][v[3]], to_device(sc["probs"][v[3]]))
        assert a.fuse_view_labels(r, sc["cams"][v[4]], mask, view_weights=spec) is None
        assert len(a._pending) == 0
        got.append(bits(a.get_raw()))
    if sc["exact"]:
        np.testing.assert_array_equal(got[0], got[1])
    want = sm.fusion.MeshAggregator(sc["P"], C, "sum", 0.5)
    want.defer = False
    for k in v[:4]:
        want.fuse_view(r, sc["cams"][k], to_device(sc["probs"][k]), None if k != v[2] else to_device(Wref[k]))
    want.fuse_view_labels(r, sc["cams"][v[4]], mask, Wref[v[4]])
    same(sc, "sum", aggs[0], want)
    same(sc, "sum", aggs[1], want)


def test_the_identity_spec_is_the_plain_call(sm):
    """ViewWeights(power=0): every visible pixel keeps its weight -- the accumulator of the plain call, in bits."""
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    d_probs = [to_device(p) for p in sc["probs"]]
    for weights in (None, sc["mine"]):
        plain, got = sm.fusion.MeshAggregator(sc["P"], C, "summax"), sm.fusion.MeshAggregator(sc["P"], C, "summax")
        plain.fuse_views(r, sc["cams"], d_probs, None if weights is None else [to_device(w) for w in weights])
        kernel = sm._lib.last_fuse_kernel()
        stats = got.fuse_views(r, sc["cams"], d_probs, weights, view_weights=sm.fusion.ViewWeights(power=0), view_stats=True)
        assert sm._lib.last_fuse_kernel() == kernel
        assert (stats[:, 0] > 0).all() and not stats[:, 1:].any()
        assert bits(plain.get_raw()).any()
        np.testing.assert_array_equal(bits(got.get_raw()), bits(plain.get_raw()))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(sm):
    from semantic_meshes_amd.device import to_device
    sc = fuse_scene(sm)
    r = sm.render.triangles(sc["mesh"])
    rt = sm.render.texels(sc["mesh"], sc["cams"], 0.05)
    spec = sm.fusion.ViewWeights(*SPEC)
    a = sm.fusion.MeshAggregator(sc["P"], C)
    a.fuse_view(r, sc["cams"][0], sc["probs"][0], view_weights=spec)
    before = bits(a.get_raw()).copy()
    assert before.any()
    a.fuse_view(r, sc["cams"][1], to_device(sc["probs"][1]))       # one deferred view: a refused call must leave it pending
    assert len(a._pending) == 1
    launches = option(sm, "view_weights_launches")
    cams, probs, sensors = sc["cams"][2:4], sc["probs"][2:4], sc["sensors"][2:4]
    gate = sm.fusion.DepthGate(0.02)
    for call in (lambda: a.fuse_views(rt, cams, probs, view_weights=spec),
                 lambda: a.fuse_views(r, cams, probs, view_weights=(2, 0.3)),
                 lambda: a.fuse_views(r, cams, probs, view_stats=True),
                 lambda: a.fuse_views(r, cams, probs, view_weights=spec, depth_stats=True),
                 lambda: a.fuse_views(r, cams, probs, view_weights=spec, sensor_depths=sensors),
                 lambda: a.fuse_views(r, cams, probs, view_weights=spec, sensor_depths=sensors[:1], depth_gate=gate),
                 lambda: a.fuse_views(r, cams, probs, resize="bilinear", sample_in_kernel=True, view_weights=spec),
                 lambda: a.fuse_view_labels(rt, cams[0], probs[0][:, :, 0].astype(np.uint8), view_weights=spec),
                 lambda: sm.fusion.view_weights_device(rt, cams[0], sc["idx"][2], sc["depth"][2], spec)):
        with pytest.raises(ValueError):
            call()
        assert len(a._pending) == 1
    # the C entry points
    lib = sm._lib.lib()
    W, H = cams[0].resolution
    d_probs, d_sensor = to_device(sc["probs"][2]), to_device(sc["sensors"][2])
    d_idx, d_depth = to_device(sc["idx"][2]), to_device(sc["depth"][2])
    out = to_device(np.zeros((W, H), np.float32))
    pods = (sm._lib.CameraPOD * 1)(cams[0]._pod)
    iptr, sptr = (ctypes.c_void_p * 1)(d_probs.ptr), (ctypes.c_void_p * 1)(d_sensor.ptr)
    handle = a._handle
    nan, inf = float("nan"), float("inf")
    good = (2, 0.3, 0, inf, inf)
    gpod = sm._lib.DepthGatePOD(0.001, 0.02, 0.0, inf, 1)

    def fuse(rh=r._h, values=good, kind=sm._lib.PROBS_F32, sensors=None, gate=None, w=W, h=H, depth_counts=None):
        pod = sm._lib.ViewWeightsPOD(*values)
        return lib.smesh_fuse_views_view_weights(rh, handle, pods, 1, iptr, kind, None, ctypes.byref(pod), sensors, sm._lib.DEPTH_U16, None,
                                                 sm._lib.MEM_DEVICE, w, h, None if gate is None else ctypes.byref(gate), None, depth_counts)

    def single(rh=r._h, values=good, w=W, h=H):
        pod = sm._lib.ViewWeightsPOD(*values)
        return lib.smesh_view_weights(rh, pods, ctypes.c_void_p(d_idx.ptr), ctypes.c_void_p(d_depth.ptr), w, h, ctypes.byref(pod), None,
                                      ctypes.c_void_p(out.ptr), None)

    bad_specs = [(-1, 0.3, 0, inf, inf), (17, 0.3, 0, inf, inf), (2, nan, 0, inf, inf), (2, -0.1, 0, inf, inf), (2, 1.5, 0, inf, inf),
                 (2, 0.3, 0, nan, inf), (2, 0.3, 0, inf, nan), (2, 0.3, 0, inf, 0.0), (2, 0.3, 0, inf, -1.0)]
    dummy = (ctypes.c_uint64 * 4)()
    for kw in ([dict(values=v) for v in bad_specs] + [dict(rh=rt._h), dict(kind=5), dict(kind=-1), dict(sensors=sptr), dict(gate=gpod),
               dict(depth_counts=dummy), dict(sensors=sptr, gate=gpod, w=0), dict(sensors=sptr, gate=gpod, h=65537),
               dict(sensors=sptr, gate=sm._lib.DepthGatePOD(nan, 0.02, 0.0, inf, 1))]):
        assert fuse(**kw) == sm._lib.ERR_INVALID, kw
        assert lib.smesh_last_error()
    for kw in [dict(values=v) for v in bad_specs] + [dict(rh=rt._h), dict(w=W + 1), dict(h=H - 1), dict(w=65537)]:
        assert single(**kw) == sm._lib.ERR_INVALID, kw
    assert lib.smesh_fuse_views_view_weights(r._h, handle, pods, 1, iptr, 0, None, None, None, 0, None, 1, 0, 0, None, None, None) == sm._lib.ERR_INVALID
    sm._lib.check(lib.smesh_synchronize(0))
    assert not out.numpy().any()
    assert option(sm, "view_weights_launches") == launches
    assert len(a._pending) == 1
    with a._pending_lock:
        a._pending = []          # drop the deferred view: what is left must be the bits from before the refused calls
    np.testing.assert_array_equal(bits(a.get_raw()), before)
    sm._lib.check(lib.smesh_synchronize(0))


# ---- the effect ------------------------------------------------------------------------------------------------------------------
def test_a_frontal_view_beats_a_grazing_one(sm):
    """A flat floor seen by a frontal camera that says class 1 and by a camera at 80 degrees that says class 2 and carries a weights
    image a thousand times larger.  Geometry alone (no code of the restatement): both cameras have a half field of view of
    atan(0.1) = 5.7 degrees, so every ray of the grazing camera meets the floor at more than 74 degrees from its normal -- a cosine
    under 0.28 -- and every ray of the frontal one at less than 6.  With power=2, min_cos=0.3 the grazing camera's pixels weigh
    nothing and the faces both cameras see carry the frontal label; without the keyword the larger weights image wins."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.data import Camera
    W, H = 160, 120
    mesh = synth.grid_mesh(40, 40, extent=4.0, relief=0.0)
    assert not np.asarray(mesh.vertices)[:, 2].any()

    def camera(tilt):
        t = math.radians(tilt)
        R, tr = synth.look_at((6.0 * math.sin(t), 0.0, 6.0 * math.cos(t)), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
        return Camera(R, tr, np.asarray([W, H]), np.asarray([5.0 * W, 5.0 * W], np.float64), np.asarray([W / 2.0, H / 2.0], np.float64))

    cams = [camera(0.0), camera(80.0)]
    r = sm.render.triangles(mesh)
    P = len(mesh.faces)
    planes = [np.asarray(r.render(cam)[0]) for cam in cams]
    seen = [np.bincount(p[p != np.uint32(0xFFFFFFFF)].astype(np.int64), minlength=P) for p in planes]
    shared = (seen[0] >= 4) & (seen[1] >= 1)
    assert shared.sum() >= 50, shared.sum()
    probs = [np.zeros((W, H, C), np.float32), np.zeros((W, H, C), np.float32)]
    probs[0][:, :, 1] = 1.0
    probs[1][:, :, 2] = 1.0
    weights = [np.ones((W, H), np.float32), np.full((W, H), 1000.0, np.float32)]
    plain, weighted = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    plain.fuse_views(r, cams, probs, weights)
    stats = weighted.fuse_views(r, cams, probs, weights, view_weights=sm.fusion.ViewWeights(power=2, min_cos=0.3), view_stats=True)
    assert (np.argmax(plain.get(), axis=1)[shared] == 2).all()
    assert (np.argmax(weighted.get(), axis=1)[shared] == 1).all()
    assert stats[0, vw.GRAZING] == 0 and stats[1, vw.GRAZING] == stats[1, vw.VISIBLE] > 0
