"""float16 / bfloat16 class-vector images on the GPU (include/smesh_half.h): every entry point against the CPU oracle fed
widen(image), with widen computed in numpy (half_helpers.py).

Where one lane owns a row -- no view of the case queues a triangle over 8 x 8 pixels -- the raw accumulator is bit-equal to the float32
single-threaded oracle and to the library's own float32 path on the widened images.  Where triangles are queued, a wave sums their
pixels in tree order; with hundreds of terms the float32 SEQUENTIAL sum itself is off by more than 1e-5 of the exact sum, so there the
reference is the oracle accumulating in float64 (what the project's room tests compare their tree-ordered paths with), within
helpers.assert_fused_close."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from half_helpers import DTYPES, describe_rows, kw, narrow, narrow_bf16, narrow_f16, random_probs16, typed, widen
from helpers import assert_fused_close, small_scene
from test_gpu_fuzz import _room
from test_gpu_labels import bits, expected_launches, fuse_slot_counts

pytestmark = pytest.mark.gpu

NATIVE = "k_fuse_tri_h16"
W, H = 160, 120
VIEWS = 15
SCENES = ("small", "odd", "room", "fine")
_cache = {}


def code_of(sm, dtype):
    return sm._lib.PROBS_F16 if dtype == "float16" else sm._lib.PROBS_BF16


def scene(sm, oracle, which):
    """(mesh, cameras, product renderer, oracle index images, queued triangles per view) -- built once per scene and left unchanged."""
    if which in _cache:
        return _cache[which]
    from semantic_meshes_amd import synth
    if which == "small":
        mesh, cams = small_scene(views=VIEWS)                      # 1 600 triangles: a multiple of 64
    elif which == "odd":
        mesh, cams = small_scene(a=37, b=19, views=VIEWS)          # 1 406 triangles: the last wave holds a partial block
        assert len(mesh.faces) % 64 != 0
    elif which == "fine":
        # 25 438 triangles of at most 4 x 4 pixels, again no multiple of 64: no view queues a triangle, so one lane owns each row and
        # the sums are the oracle's bit for bit (the two coarse grids above have boxes of up to 15 pixels: some triangles are queued)
        mesh, cams = small_scene(a=161, b=79, views=VIEWS)
        assert len(mesh.faces) % 64 != 0
    else:
        rng = np.random.default_rng(4242)
        verts, faces, half = _room(rng, 8)                         # seen from inside: queued big triangles, near-plane clipping
        mesh, cams = types.SimpleNamespace(vertices=verts, faces=faces), []
        for _ in range(VIEWS):
            eye = rng.uniform(-0.85, 0.85, 3) * half
            target = rng.uniform(-1.0, 1.0, 3) * half
            R, t = synth.look_at(tuple(eye), tuple(target), up=(0, 0, 1))
            f = float(rng.uniform(0.35, 1.2)) * W
            cams.append(sm.data.Camera(R, t, np.array([W, H]), np.array([f, f]), np.array([W / 2.0, H / 2.0])))
    r = sm.render.triangles(mesh)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    oidx, queued = [], []
    for cam in cams:
        oi = o.render(cam)[0]
        np.testing.assert_array_equal(np.asarray(r.render(cam)[0]), oi)
        queued.append(int(r.render_stats(cam, queues=True)[1][0]))
        oidx.append(oi)
    if which == "room":
        assert sum(queued) > 0
    if which == "fine":
        assert sum(queued) == 0
    _cache[which] = (mesh, cams, r, oidx, queued)
    return _cache[which]


def images(C, dtype, n=VIEWS, seed=0):
    """`n` test images of one class count and dtype as uint16 bit patterns, generated once; their widened copies beside them."""
    key = ("img", C, dtype, n, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * C + 7 * DTYPES.index(dtype) + seed)
        img = [random_probs16(rng, W, H, C, dtype) for _ in range(n)]
        zero, below, above, sub = map(sum, zip(*[describe_rows(i, dtype) for i in img]))
        assert zero > 0 and below > 0 and above > 0                # don't-care rows; widened sums on either side of 0.5
        if dtype == "float16" and C >= 19:
            assert sub > 0                                         # binary16 subnormals: most classes of most pixels
        _cache[key] = (img, [widen(i, dtype) for i in img])
    return _cache[key]


def device_images(sm, img, dtype):
    from semantic_meshes_amd.device import to_device
    out = [to_device(typed(i, dtype)) for i in img]
    return out


def oracle_raw(oracle, P, C, kind, iew, oidx, wide, weights=None, double=False, views=None):
    oracle.set_accum_double(double)
    try:
        oagg = oracle.OracleAggregator(P, C, kind, iew)
        for k in (range(len(oidx)) if views is None else views):
            oagg.add(oidx[k], wide[k], None if weights is None else weights[k])
        return oagg.get_raw(), oagg.get()
    finally:
        oracle.set_accum_double(False)


def check_against_oracle(oracle, agg, P, C, kind, iew, oidx, wide, queued, weights=None, views=None):
    got = agg.get_raw()
    assert np.abs(got).sum() > 0
    if queued == 0:
        want, dist = oracle_raw(oracle, P, C, kind, iew, oidx, wide, weights, views=views)
        np.testing.assert_array_equal(bits(got), bits(want))
        np.testing.assert_array_equal(bits(agg.get()), bits(dist))
    else:
        want64, dist64 = oracle_raw(oracle, P, C, kind, iew, oidx, wide, weights, double=True, views=views)
        print("    queued=%d max|raw - float64-accumulating oracle|=%g" % (queued, np.nanmax(np.abs(got.astype(np.float64) - want64))))
        assert_fused_close(got, want64)
        assert_fused_close(agg.get(), dist64)
    return got


# ---- 1. the native kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SCENES)
@pytest.mark.parametrize("C", [5, 8, 19, 40, 48])
@pytest.mark.parametrize("kind", ["sum", "summax"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_native_kernel_against_the_oracle(sm, oracle, dtype, kind, C, which):
    from semantic_meshes_amd.device import to_device
    mesh, cams, r, oidx, queued = scene(sm, oracle, which)
    P = len(mesh.faces)
    img, wide = images(C, dtype)
    iew = [0.0, 0.5, 1.0][(C + len(kind)) % 3]
    agg = sm.fusion.MeshAggregator(P, C, kind, iew)
    d16 = device_images(sm, img, dtype)
    launches, fused = fuse_slot_counts(sm, lambda: agg.fuse_views(r, cams, d16, **kw(dtype)))
    assert sm._lib.last_fuse_kernel() == NATIVE
    assert sm._lib.get_option("last_fuse_probs_dtype") == code_of(sm, dtype)
    cap = max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8")))
    print("    %d launches for %d views, at most %d per launch" % (launches, fused, cap))
    assert fused == VIEWS and launches == expected_launches(VIEWS, cap), (launches, fused, cap)     # 8 + 4 + 2 + 1 views
    got = check_against_oracle(oracle, agg, P, C, kind, iew, oidx, wide, sum(queued))
    if sum(queued) == 0:
        ref = sm.fusion.MeshAggregator(P, C, kind, iew)      # the library's own float32 path on the widened images
        ref.fuse_views(r, cams, [to_device(w) for w in wide])
        assert sm._lib.last_fuse_kernel() == "k_fuse_tri" and sm._lib.get_option("last_fuse_probs_dtype") == 0
        np.testing.assert_array_equal(bits(got), bits(ref.get_raw()))


# ---- 2. weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["odd", "room", "fine"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_with_zeros_on_all_and_on_some_views(sm, oracle, dtype, which):
    from semantic_meshes_amd.device import to_device
    C, kind, iew = 19, "sum", 0.5
    mesh, cams, r, oidx, queued = scene(sm, oracle, which)
    P = len(mesh.faces)
    img, wide = images(C, dtype)
    rng = np.random.default_rng(77)
    weights = []
    for _ in cams:
        w = rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32)
        w[rng.random((W, H)) < 0.2] = 0.0
        weights.append(w)
    d16 = device_images(sm, img, dtype)
    agg = sm.fusion.MeshAggregator(P, C, kind, iew)
    agg.fuse_views(r, cams, d16, [to_device(w) for w in weights], **kw(dtype))
    assert sm._lib.last_fuse_kernel() == NATIVE
    check_against_oracle(oracle, agg, P, C, kind, iew, oidx, wide, sum(queued), weights)
    some = [w if k % 3 else None for k, w in enumerate(weights)]                # weights on only some views of the batch
    agg = sm.fusion.MeshAggregator(P, C, kind, iew)
    agg.fuse_views(r, cams, d16, [None if w is None else to_device(w) for w in some], **kw(dtype))
    assert sm._lib.last_fuse_kernel() == NATIVE
    check_against_oracle(oracle, agg, P, C, kind, iew, oidx, wide, sum(queued), some)


# ---- 3. strided images ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [19, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_network_output_seen_as_whc_is_fused_in_place(sm, oracle, dtype, C):
    from semantic_meshes_amd.device import to_device
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=5, seed=3)
    dense, strided = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    for k in range(5):
        dense.add(r.render(cams[k])[0], to_device(typed(img[k], dtype)), **kw(dtype))
        hwc = to_device(typed(np.ascontiguousarray(img[k].transpose(1, 0, 2)), dtype))       # (H,W,C), as a network leaves it
        view = hwc.transpose(1, 0, 2)                                                          # (W,H,C) at strides (C, W * C, 1)
        assert view.shape == (W, H, C) and view.strides == (C, W * C, 1)
        strided.add(r.render(cams[k])[0], view, **kw(dtype))
        assert sm._lib.last_fuse_kernel() == NATIVE and sm._lib.last_add_path() == "render-records"
    got = check_against_oracle(oracle, strided, P, C, "sum", 0.5, oidx, wide, 0, views=range(5))
    np.testing.assert_array_equal(bits(got), bits(dense.get_raw()))


# ---- 3b. every instance, by the reported slot and view count -------------------------------------------------------------------------
def _boxes(mesh, cams, oidx):
    """Per view of the "odd" scene: the triangles SURELY queued (their visible pixels alone span more than 8 in x or y) and the
    triangles SURELY not (the projected vertices span at most 5 pixels either way: at most six pixel columns, eight with a pixel of
    padding on both sides), both from the CPU side only -- the oracle's index images and the pinhole projection in float64."""
    key = ("boxes", len(mesh.faces), len(cams))
    if key in _cache:
        return _cache[key]
    P = len(mesh.faces)
    v = np.asarray(mesh.vertices, np.float64)
    tri = np.asarray(mesh.faces)
    big, small = [], []
    for cam, oi in zip(cams, oidx):
        pc = v @ cam.rotation.astype(np.float64).T + cam.translation.astype(np.float64)
        assert (pc[:, 2] > 0).all()                                # seen from outside: nothing near the camera plane
        uv = pc[:, :2] / pc[:, 2:3] * cam.focal_lengths + cam.principal_point
        ext = (uv[tri].max(axis=1) - uv[tri].min(axis=1)).max(axis=1)
        small.append(ext <= 5.0)
        x, y = np.nonzero(oi < P)
        f = oi[x, y]
        lo = np.full((P, 2), 1 << 30)
        hi = np.full((P, 2), -1)
        for axis, coord in enumerate((x, y)):
            np.minimum.at(lo[:, axis], f, coord)
            np.maximum.at(hi[:, axis], f, coord)
        big.append(((hi - lo + 1) > 8).any(axis=1) & (hi[:, 0] >= 0))
    _cache[key] = (np.array(big), np.array(small))
    return _cache[key]


def _fuse_and_report(sm, oracle, which, C, dtype, kind, n, weighted):
    """`n` views of a scene through k_fuse_tri_h16, checked as test_native_kernel_against_the_oracle checks them: bit-equal to the oracle
    and to the float32 path on the widened images where no view queues a triangle, else within helpers.assert_fused_close of the
    float64-accumulating oracle (a wave sums a queued triangle's pixels in tree order here, the medium and big triangle paths of
    k_fuse_tri in theirs there).  Returns the reported (slot, views) of the last launch."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, r, oidx, queued = scene(sm, oracle, which)
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=n, seed=2)
    weights = None
    if weighted:
        rng = np.random.default_rng(99)
        weights = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) if k % 2 == 0 else None for k in range(n)]   # view 0 has one
    d_w = None if weights is None else [None if w is None else to_device(w) for w in weights]
    agg = sm.fusion.MeshAggregator(P, C, kind)
    agg.fuse_views(r, cams[:n], device_images(sm, img, dtype), d_w, **kw(dtype))
    assert sm._lib.last_fuse_kernel() == NATIVE
    instance = sm._lib.get_option("last_fuse_slot"), sm._lib.get_option("last_fuse_views")
    got = check_against_oracle(oracle, agg, P, C, kind, 0.5, oidx[:n], wide, sum(queued[:n]), weights)
    if sum(queued[:n]) == 0:
        ref = sm.fusion.MeshAggregator(P, C, kind)
        ref.fuse_views(r, cams[:n], [to_device(w) for w in wide], d_w)
        assert sm._lib.last_fuse_kernel() == "k_fuse_tri"
        np.testing.assert_array_equal(bits(got), bits(ref.get_raw()))
    return instance


@pytest.mark.parametrize("C", [1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48])
def test_every_slot_edge(sm, oracle, C):
    """The class counts around every register-slot boundary of k_fuse_tri_h16, where the tail piece of a row load can go wrong
    (test_gpu_sampled.py::test_every_slot_edge for this kernel).  On "fine", the smallest scene without queued triangles: only there
    are the sums bit-equal to the float32 path's."""
    dtype = DTYPES[(C // 8 + C) % 2]                                 # one of the two per class count, both on either side of an edge
    kind = "summax" if C % 2 else "sum"
    slot, views = _fuse_and_report(sm, oracle, "fine", C, dtype, kind, 3, False)
    assert slot == (C + 7) // 8 * 8 and views == 1                   # the last launch of 2 + 1


@pytest.mark.parametrize("n,last", [(1, 1), (2, 2), (3, 1), (4, 4), (8, 8)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_view_count(sm, oracle, dtype, n, last):
    """Every view count of the kernel on the "odd" scene: a last, partial block of rows, triangles that one view of a launch queues and
    another does not (the tail wave then takes them in every view), and weights images on some views."""
    assert max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8"))) >= 8
    mesh, cams, r, oidx, queued = scene(sm, oracle, "odd")
    assert len(mesh.faces) % 64 != 0
    big, small = _boxes(mesh, cams, oidx)
    assert (big[:8].any(axis=0) & small[:8].any(axis=0)).any() and big[0].any()
    assert _fuse_and_report(sm, oracle, "odd", 19, dtype, "sum", n, True) == (24, last)


# ---- 4. the widening route ----------------------------------------------------------------------------------------------------------
def _widened_kernel(sm):
    kernel = sm._lib.last_fuse_kernel()
    assert kernel not in (NATIVE, "none") and sm._lib.get_option("last_fuse_probs_dtype") == 0, kernel
    return kernel


@pytest.mark.parametrize("dtype", DTYPES)
def test_widening_route_mul(sm, oracle, dtype):
    """Mul as the existing Mul tests check it: strictly positive class vectors, get() against the float64-accumulating oracle."""
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    rng = np.random.default_rng(5)
    img = []
    for _ in range(4):
        p = widen(random_probs16(rng, W, H, C, dtype), dtype)
        p = np.where(p.sum(-1, keepdims=True) > 0, np.maximum(p, 1e-3), 0).astype(np.float32)
        img.append(narrow(p, dtype))
    wide = [widen(i, dtype) for i in img]
    agg = sm.fusion.MeshAggregator(P, C, "mul")
    agg.fuse_views(r, cams[:4], device_images(sm, img, dtype), **kw(dtype))
    _widened_kernel(sm)
    want = oracle_raw(oracle, P, C, "mul", 0.5, oidx[:4], wide, double=True)[1]
    assert_fused_close(agg.get(), want, rtol=1e-5, atol=1e-6)
    ref = sm.fusion.MeshAggregator(P, C, "mul")
    ref.fuse_views(r, cams[:4], [to_device(w) for w in wide])
    assert_fused_close(agg.get(), ref.get(), rtol=1e-6)      # (the (hi, lo) pairs fold once per view either way: test_gpu_deferred's bound)


@pytest.mark.parametrize("C", [49, 150])
@pytest.mark.parametrize("dtype", DTYPES)
def test_widening_route_more_classes_than_the_kernel_serves(sm, oracle, dtype, C):
    from semantic_meshes_amd.device import to_device
    assert sm._lib.get_option("half_max_classes") == 48
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=3, seed=1)
    agg = sm.fusion.MeshAggregator(P, C, "summax")
    agg.fuse_views(r, cams[:3], device_images(sm, img, dtype), **kw(dtype))
    kernel = _widened_kernel(sm)
    want64, dist64 = oracle_raw(oracle, P, C, "summax", 0.5, oidx[:3], wide, double=True)
    assert_fused_close(agg.get_raw(), want64)
    assert_fused_close(agg.get(), dist64)
    ref = sm.fusion.MeshAggregator(P, C, "summax")           # the same float32 kernel on the widened images, view by view
    for k in range(3):
        ref.fuse_view(r, cams[k], to_device(wide[k]))
    assert sm._lib.last_fuse_kernel() == kernel
    np.testing.assert_array_equal(bits(agg.get_raw()), bits(ref.get_raw()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_widening_route_texel_renderer(sm, oracle, dtype):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
    img, wide = images(C, dtype, n=3, seed=1)
    rt = sm.render.texels(mesh, cams[:3], 0.05)
    ot = oracle.OracleRenderer(mesh.vertices, mesh.faces, cams[:3], 0.05)
    P = rt.getPrimitivesNum()
    agg, one = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    agg.fuse_views(rt, cams[:3], device_images(sm, img, dtype), **kw(dtype))
    _widened_kernel(sm)
    tidx = [ot.render(cam)[0] for cam in cams[:3]]
    want64, dist64 = oracle_raw(oracle, P, C, "sum", 0.5, tidx, wide, double=True)
    assert_fused_close(agg.get_raw(), want64)
    assert_fused_close(agg.get(), dist64)
    for k in range(3):
        one.add(rt.render(cams[k])[0], device_images(sm, img[k:k + 1], dtype)[0], **kw(dtype))
        _widened_kernel(sm)
    assert_fused_close(one.get_raw(), want64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_widening_route_foreign_index_image(sm, oracle, dtype):
    """add() on a numpy index image: nobody's render, so the image is widened and takes add()'s own path."""
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=3, seed=1)
    foreign = []
    for k in range(3):
        idx = oidx[k].copy()
        idx[3, 5] = 0 if idx[3, 5] != 0 else 1
        foreign.append(idx)
    host, dev = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    for k in range(3):
        host.add(foreign[k], typed(img[k], dtype), **kw(dtype))               # host index image, host 16-bit image
        _widened_kernel(sm)
        dev.add(foreign[k], device_images(sm, img[k:k + 1], dtype)[0], **kw(dtype))
        _widened_kernel(sm)
    want64, dist64 = oracle_raw(oracle, P, C, "sum", 0.5, foreign, wide, double=True)
    for agg in (host, dev):
        assert_fused_close(agg.get_raw(), want64)
        assert_fused_close(agg.get(), dist64)
    assert_fused_close(host.get_raw(), dev.get_raw())      # (the moved pixel makes primitive 0 a sparse one: float atomics, no fixed order)


def _child(test_name, **env):
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", test_name, "-p",
                          "no:cacheprovider"], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def _native_or_widened_case(sm, oracle, expect_native):
    for dtype in DTYPES:
        C = 19
        mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
        P = len(mesh.faces)
        img, wide = images(C, dtype, n=3, seed=1)
        agg = sm.fusion.MeshAggregator(P, C)
        agg.fuse_views(r, cams[:3], device_images(sm, img, dtype), **kw(dtype))
        kernel = sm._lib.last_fuse_kernel()
        assert (kernel == NATIVE) == expect_native, kernel
        if not expect_native:
            _widened_kernel(sm)
        want64, dist64 = oracle_raw(oracle, P, C, "sum", 0.5, oidx[:3], wide, double=True)
        assert_fused_close(agg.get_raw(), want64)
        one = sm.fusion.MeshAggregator(P, C)
        for k in range(3):
            one.add(r.render(cams[k])[0], device_images(sm, img[k:k + 1], dtype)[0], **kw(dtype))
        assert (sm._lib.last_fuse_kernel() == NATIVE) == expect_native
        assert_fused_close(one.get_raw(), want64)


def test_widening_route_reordered_mesh_child(sm, oracle):
    """SMESH_REORDER=1 (read when the renderer is made): rows are not in triangle order, the 16-bit kernel does not serve them."""
    if os.environ.get("SMESH_REORDER") != "1":
        _child("test_widening_route_reordered_mesh_child", SMESH_REORDER="1")
        return
    _native_or_widened_case(sm, oracle, expect_native=False)


def test_widening_route_forced_by_the_hook_child(sm, oracle):
    """SMESH_FUSE_H16=0 in the environment of a process: every 16-bit image takes the widening route."""
    if os.environ.get("SMESH_FUSE_H16") != "0":
        _native_or_widened_case(sm, oracle, expect_native=True)
        _child("test_widening_route_forced_by_the_hook_child", SMESH_FUSE_H16="0")
        return
    _native_or_widened_case(sm, oracle, expect_native=False)


# ---- 5. host images ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_images_equal_device_images(sm, oracle, dtype):
    """float16 numpy arrays, and uint16 + probs_dtype="bfloat16", through add, fuse_view and fuse_views: the device images' bits."""
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=10, seed=2)
    cams10, host = cams[:10], [typed(i, dtype) for i in img]
    assert host[0].dtype == (np.float16 if dtype == "float16" else np.uint16)
    rng = np.random.default_rng(3)
    weights = [rng.uniform(0.0, 2.0, size=(W, H)).astype(np.float32) for _ in cams10]
    dev = sm.fusion.MeshAggregator(P, C)
    dev.fuse_views(r, cams10, device_images(sm, img, dtype), **kw(dtype))
    want = check_against_oracle(oracle, dev, P, C, "sum", 0.5, oidx[:10], wide, 0)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_views(r, cams10, host, **kw(dtype))                    # ten views: a group of eight and one of two through the staging scratch
    assert sm._lib.last_fuse_kernel() == NATIVE
    np.testing.assert_array_equal(bits(a.get_raw()), bits(want))
    a = sm.fusion.MeshAggregator(P, C)
    for cam, h in zip(cams10, host):
        a.fuse_view(r, cam, h, **kw(dtype))
    assert sm._lib.last_fuse_kernel() == NATIVE
    np.testing.assert_array_equal(bits(a.get_raw()), bits(want))
    a = sm.fusion.MeshAggregator(P, C)
    for cam, h in zip(cams10, host):
        a.add(r.render(cam)[0], h, **kw(dtype))
    assert sm._lib.last_fuse_kernel() == NATIVE
    np.testing.assert_array_equal(bits(a.get_raw()), bits(want))
    # ... and with host weights
    a, b = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    a.fuse_views(r, cams10, host, weights, **kw(dtype))
    for cam, h, w in zip(cams10, host, weights):
        b.add(r.render(cam)[0], h, w, **kw(dtype))
    got = check_against_oracle(oracle, a, P, C, "sum", 0.5, oidx[:10], wide, 0, weights)
    np.testing.assert_array_equal(bits(b.get_raw()), bits(got))


# ---- 6. the reference's loop ------------------------------------------------------------------------------------------------------
def test_render_add_loop_is_deferred_into_one_eight_view_launch(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    for dtype in DTYPES:
        img, wide = images(C, dtype, n=8, seed=4)
        d16 = device_images(sm, img, dtype)
        if dtype == "bfloat16":
            for d in d16:
                d.bfloat16 = True          # (what narrow_probs' result says of itself: no keyword needed)
        agg = sm.fusion.MeshAggregator(P, C)
        assert agg.defer

        def loop():
            for k in range(8):
                idx, depth = r.render(cams[k])
                agg.add(idx, d16[k])
                assert idx.unrun and len(agg._pending) == (k + 1) % 8
        launches, fused = fuse_slot_counts(sm, loop)
        assert sm._lib.last_fuse_kernel() == NATIVE and sm._lib.get_option("last_fuse_probs_dtype") == code_of(sm, dtype)
        cap = max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8")))
        assert (launches, fused) == (expected_launches(8, cap), 8)            # one launch of eight views
        want = check_against_oracle(oracle, agg, P, C, "sum", 0.5, oidx[:8], wide, 0)
        per_call = sm.fusion.MeshAggregator(P, C)
        per_call.defer = False
        for k in range(8):
            idx, depth = r.render(cams[k])
            per_call.add(idx, d16[k])
            assert not idx.unrun
        assert sm._lib.last_fuse_kernel() == NATIVE
        np.testing.assert_array_equal(bits(per_call.get_raw()), bits(want))


def test_a_dtype_change_flushes_the_deferred_group(sm, oracle):
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    f16, wide16 = images(C, "float16", n=9, seed=4)
    b16, wideb = images(C, "bfloat16", n=9, seed=4)
    order = ["float16"] * 3 + ["bfloat16"] * 2 + ["float32"] * 2 + ["float16"] * 2
    agg = sm.fusion.MeshAggregator(P, C)
    wide, pending = [], []
    for k, dt in enumerate(order):
        if dt == "float16":
            d, w = to_device(typed(f16[k], dt)), wide16[k]
        elif dt == "bfloat16":
            d, w = to_device(b16[k]), wideb[k]
        else:
            d, w = to_device(wide16[k]), wide16[k]
        agg.add(r.render(cams[k])[0], d, **kw(dt))
        wide.append(w)
        pending.append(len(agg._pending))
    assert pending == [1, 2, 3, 1, 2, 1, 2, 1, 2]                 # a change of dtype hands the group over, like a change of size
    check_against_oracle(oracle, agg, P, C, "sum", 0.5, oidx[:9], wide, 0)


def test_the_loop_without_deferred_views_child(sm, oracle):
    """SMESH_DEFER_VIEWS=0 (read at import): the same loops, every view consumed by its own call."""
    if os.environ.get("SMESH_DEFER_VIEWS") != "0":
        _child("test_the_loop_without_deferred_views_child", SMESH_DEFER_VIEWS="0")
        return
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    for dtype in DTYPES:
        img, wide = images(C, dtype, n=8, seed=4)
        d16 = device_images(sm, img, dtype)
        agg = sm.fusion.MeshAggregator(P, C)
        assert not agg.defer
        for k in range(8):
            idx, depth = r.render(cams[k])
            agg.add(idx, d16[k], **kw(dtype))
            assert not agg._pending and not idx.unrun
        assert sm._lib.last_fuse_kernel() == NATIVE
        check_against_oracle(oracle, agg, P, C, "sum", 0.5, oidx[:8], wide, 0)


# ---- 7. add_many ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_many_with_rendered_index_planes(sm, oracle, dtype):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    img, wide = images(C, dtype, n=11, seed=6)
    agg = sm.fusion.MeshAggregator(P, C, "summax")
    planes = [r.render(cam)[0] for cam in cams[:11]]
    launches, fused = fuse_slot_counts(sm, lambda: (agg.add_many(planes, device_images(sm, img, dtype), **kw(dtype)), agg.flush()))
    assert sm._lib.last_fuse_kernel() == NATIVE
    assert fused == 11 and launches == expected_launches(8, 8) + expected_launches(3, 8)
    check_against_oracle(oracle, agg, P, C, "summax", 0.5, oidx[:11], wide, 0)


# ---- 8. narrowing -----------------------------------------------------------------------------------------------------------------
def test_narrowing_on_the_device_is_round_to_nearest_even(sm):
    from semantic_meshes_amd import synth
    rng = np.random.default_rng(8)
    x = rng.integers(0, 1 << 32, size=100_003, dtype=np.uint64).astype(np.uint32).view(np.float32)     # every exponent, not a multiple of 4
    x = x[~np.isnan(x)]
    special = np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, 65519.0, 65520.0, 1e5, -1e5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                        3 * 2.0 ** -25, 6.0e-5, 6.1e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                        3.4e38, -3.4e38, 1e-40, 2.0 ** -134], np.float32)
    ties16 = (np.arange(0, 2048, dtype=np.uint32) << 13 | 0x38001000).view(np.float32)       # binary16 ties in [2^-15, 2^-14) ...
    sub16 = (rng.random(4096) * 6.1e-5).astype(np.float32)                                     # ... and values that narrow to subnormals
    tiesb = (np.arange(0, 4096, dtype=np.uint32) << 16 | 0x3F008000).view(np.float32)        # bfloat16 ties
    x = np.concatenate([special, ties16, sub16, tiesb, x])
    got16 = sm.fusion.narrow_probs(x, "float16")
    assert got16.dtype == np.float16 and not got16.bfloat16 and got16.shape == x.shape
    np.testing.assert_array_equal(np.asarray(got16).view(np.uint16), narrow_f16(x))
    gotb = sm.fusion.narrow_probs(x, "bfloat16")
    assert gotb.dtype == np.uint16 and gotb.bfloat16
    np.testing.assert_array_equal(np.asarray(gotb), narrow_bf16(x))
    nan = sm.fusion.narrow_probs(np.array([np.nan, 1.0], np.float32), "bfloat16")
    assert np.isnan(widen(np.asarray(nan), "bfloat16")[0]) and np.asarray(nan)[1] == 0x3F80
    assert np.isnan(np.asarray(sm.fusion.narrow_probs(np.array([np.nan], np.float32), np.float16))[0])
    # host memory through the C entry point
    out = np.zeros(len(x), np.uint16)
    sm._lib.check(sm._lib.lib().smesh_narrow_probs(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), len(x),
                                                   sm._lib.PROBS_F16, 0, sm._lib.MEM_HOST))
    np.testing.assert_array_equal(out, narrow_f16(x))
    # synth.device_probs(dtype=...) narrows the float32 image it would have returned
    f32 = np.asarray(synth.device_probs(64, 48, 19, 11, 0.05, 0))
    np.testing.assert_array_equal(np.asarray(synth.device_probs(64, 48, 19, 11, 0.05, 0, dtype=np.float16)).view(np.uint16), narrow_f16(f32))
    np.testing.assert_array_equal(np.asarray(synth.device_probs(64, 48, 19, 11, 0.05, 0, dtype="bfloat16")), narrow_bf16(f32))


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_aggregator_unchanged(sm, oracle):
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
    P = len(mesh.faces)
    img, wide = images(C, "float16", n=3, seed=1)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view(r, cams[0], to_device(typed(img[0], "float16")))
    before = bits(a.get_raw()).copy()
    assert before.any()
    d64, d16, d32, u16 = to_device(wide[1].astype(np.float64)), to_device(typed(img[1], "float16")), to_device(wide[1]), to_device(img[1])
    for bad, kwargs in ((d64, {}), (d16, {"probs_dtype": "bfloat16"}), (d32, {"probs_dtype": "bfloat16"}), (u16, {}),
                        (to_device(typed(img[1][:, :-1], "float16")), {})):
        with pytest.raises(ValueError):
            a.add(r.render(cams[1])[0], bad, **kwargs)
        with pytest.raises(ValueError):
            a.fuse_view(r, cams[1], bad, **kwargs)
        with pytest.raises(ValueError):
            a.fuse_views(r, [cams[1]], [bad], **kwargs)
    with pytest.raises(ValueError, match="one dtype"):
        a.fuse_views(r, cams[1:3], [d16, d32])
    with pytest.raises(ValueError, match="one dtype"):
        a.add_many([r.render(cams[1])[0], r.render(cams[2])[0]], [d16, d32])
    lib = sm._lib.lib()
    for code in (sm._lib.PROBS_F32, 3, -1):      # a bad dtype code through the C entry points
        ptrs = (ctypes.c_void_p * 1)(d16.ptr)
        pods = (sm._lib.CameraPOD * 1)(cams[1]._pod)
        for status in (lib.smesh_fuse_view_probs16(r._h, a._h, ctypes.byref(cams[1]._pod), ctypes.c_void_p(d16.ptr), code, None, sm._lib.MEM_DEVICE),
                       lib.smesh_fuse_views_probs16(r._h, a._h, pods, 1, ptrs, code, None, sm._lib.MEM_DEVICE),
                       lib.smesh_aggregator_add_probs16(a._h, None, oidx[1].ctypes.data_as(ctypes.c_void_p), sm._lib.IDX_U32, None, sm._lib.MEM_HOST,
                                                        ctypes.c_void_p(d16.ptr), code, None, sm._lib.MEM_DEVICE, None, None, sm._lib.MEM_HOST, W, H)):
            assert status == sm._lib.ERR_INVALID and lib.smesh_last_error()
            with pytest.raises(ValueError):
                sm._lib.check(status)
    status = lib.smesh_aggregator_add_probs16(a._h, None, oidx[1].ctypes.data_as(ctypes.c_void_p), sm._lib.IDX_U32, None, sm._lib.MEM_HOST,
                                              ctypes.c_void_p(d16.ptr), sm._lib.PROBS_F16, (ctypes.c_int64 * 3)(H * C, -C, 1), sm._lib.MEM_DEVICE,
                                              None, None, sm._lib.MEM_HOST, W, H)
    assert status == sm._lib.ERR_INVALID and b"stride" in lib.smesh_last_error()
    np.testing.assert_array_equal(bits(a.get_raw()), before)
