"""Label images at their own resolution and in the dataset's ids on the GPU (include/smesh_label_prep.h): `prepare_labels` against
label_prep_ref, exact; every fusion entry point with `resize=` / `label_map=` against the CPU oracle fed one_hot of the
reference-prepared mask -- bit for bit where one lane owns a row --; the fallback routes, the order of additions, the pass-through,
ground truth with `gt_resize=` / `gt_map=`, and the refusals."""
import ctypes
import types

import numpy as np
import pytest

import label_prep_ref as lp
import resize_ref as ref
from helpers import assert_fused_close, small_scene
from test_gpu_fuzz import _room
from test_labels_host import one_hot
from test_sampled_host import VIEWS, fine_index_images

pytestmark = pytest.mark.gpu

NATIVE = "k_fuse_tri_labels"
W, H = 160, 120
SHAPES = ref.SHAPES + lp.EXTRA_SHAPES
DTYPES = (np.uint8, np.int8, np.uint16, np.int32, np.int64)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def option(sm, name):
    return sm._lib.get_option(name)


def layouts(src, device):
    """The (w,h) image dense, as the transposed view of an (h,w) array, and at strides larger than dense on both axes -- on the host
    or in device memory."""
    from semantic_meshes_amd.device import DeviceArray, to_device
    w, h = src.shape
    big = np.zeros((2 * w + 1, 3 * h + 2), src.dtype)
    big[1:1 + 2 * w:2, 2:2 + 3 * h:3] = src
    if not device:
        return {"dense": src, "transposed": np.ascontiguousarray(src.T).T, "strided": big[1:1 + 2 * w:2, 2:2 + 3 * h:3]}
    dbig = to_device(big)
    pitch = big.shape[1]
    return {"dense": to_device(src), "transposed": to_device(np.ascontiguousarray(src.T)).T,
            "strided": DeviceArray(dbig.ptr + (pitch + 2) * src.dtype.itemsize, (w, h), src.dtype, dbig.device, (2 * pitch, 3), owner=dbig)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_prepare_labels_equals_the_restatement(sm, shape):
    """Every source dtype, layout and memory, with and without a map (7 entries with -1 and values >= C inside; 1 358 entries, which
    the kernel keeps in LDS; more entries than it keeps there), source values negative and >= M, a uint8 and a uint16 plane: the bytes
    of label_prep_ref.prepare.  (The issue's "tiles on and off" leg went with the tiled form of the kernel, which the bench's decision
    rule removed together with its option: DESIGN.md 3.10.  A host view whose span is over twice its size is made dense by describe()
    first, so the strided layout reaches the kernel from device memory only.)"""
    (w, h), size = shape
    lds_max = option(sm, "labels_prepare_map_lds_max")
    assert lds_max == sm._lib.LABEL_PREP_MAP_LDS_MAX
    rng = np.random.default_rng(1000 * w + h)
    calls = 0
    for C in (5, 300):
        short = np.array([2, -1, C, 0, C + 7, C - 1, 1], np.int32)
        assert len(short) == 7 and (short == -1).any() and (short >= C).any()
        maps = {"none": None, "short": short, "scannet": lp.make_map(rng, 1358, C), "global": lp.make_map(rng, lds_max + 904, C)}
        for dtype in DTYPES:
            for name, m in maps.items():
                top = C if m is None else len(m)
                src = lp.make_source(rng, w, h, dtype, top)
                want = lp.prepare(src, C, size, m)
                assert want.dtype == (np.uint8 if C <= 255 else np.uint16)
                for device in (False, True):
                    for layout, image in layouts(src, device).items():
                        before = option(sm, "labels_prepare_launches")
                        out = sm.fusion.prepare_labels(image, C, size, "nearest", m)
                        assert option(sm, "labels_prepare_launches") - before == 1
                        calls += 1
                        np.testing.assert_array_equal(out, want, err_msg="%s %s %s device=%s C=%d" % (np.dtype(dtype).name, name, layout, device, C))
    print("    %d calls" % calls)


def test_prepare_labels_forms(sm):
    """One dimension is (n, 1); a device map; the device result; the identity without keywords."""
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(5)
    m = lp.make_map(rng, 50, 7)
    v = lp.make_source(rng, 33, 1, np.int16, 50)[:, 0]
    want = lp.prepare(v.reshape(-1, 1), 7, None, m)
    np.testing.assert_array_equal(sm.fusion.prepare_labels(v, 7, label_map=m), want)
    d = sm.fusion.prepare_labels_device(to_device(v), 7, label_map=to_device(m))
    assert d.shape == (33, 1) and d.dtype == np.uint8
    np.testing.assert_array_equal(d.numpy(), want)
    x = lp.make_source(rng, 9, 4, np.int32, 300)
    np.testing.assert_array_equal(sm.fusion.prepare_labels(x, 300), lp.prepare(x, 300))
    with pytest.raises(ValueError, match='resize="nearest"'):
        sm.fusion.prepare_labels(x, 300, (18, 8))


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
def fine_scene(sm, oracle):
    """test_gpu_half's "fine" scene at 160 x 120: every triangle box at most 8 x 8 pixels in each of its first 11 views, so one lane
    owns each accumulator row and the float32 oracle is the reference for bit equality."""
    if "fine" not in _cache:
        mesh, cams = small_scene(a=161, b=79, views=VIEWS)
        cams = cams[:11]
        P, oidx = fine_index_images(oracle)
        r = sm.render.triangles(mesh)
        for k, cam in enumerate(cams):
            np.testing.assert_array_equal(np.asarray(r.render(cam)[0]), oidx[k])
            assert r.render_stats(cam, queues=True)[1][0] == 0      # no queued triangle: the condition for bit equality
        _cache["fine"] = (mesh, cams, P, oidx[:11])
    return _cache["fine"]


def fusion_inputs(size, C, with_map, n):
    """n source masks of FUSION_SOURCES[size] and the map (64 entries, or None), generated once per key and left unchanged, with the
    reference-prepared (160,120) planes."""
    key = ("masks", size, C, with_map, n)
    if key not in _cache:
        w, h = lp.FUSION_SOURCES[size]
        rng = np.random.default_rng(17 * w + 3 * C + int(with_map))
        m = lp.make_map(rng, 64, C) if with_map else None
        masks = [lp.make_source(rng, w, h, np.int32, 64 if with_map else C) for _ in range(n)]
        _cache[key] = (masks, m, [lp.prepare(x, C, (W, H), m) for x in masks])
    return _cache[key]


FUSION_CASES = [(size, kind, C, with_map) for size in sorted(lp.FUSION_SOURCES) for kind in ("sum", "summax") for C in (5, 19, 150, 300)
                for with_map in (False, True)]


def dealt(case):
    """(with weights, iew, how the masks are handed over) of a fusion case, dealt round so that every value meets every source size,
    kind, class count and both map settings."""
    i = FUSION_CASES.index(case)
    si_, ki, ci, mi = i // 16, (i // 8) % 2, (i // 2) % 4, i % 2
    return bool((si_ + ki + ci + mi) % 2), (0.0, 0.5, 1.0)[(si_ + 2 * ki + ci + mi) % 3], ("host", "device", "transposed")[(si_ + ki + mi) % 3]


def test_the_fusion_cases_are_dealt_evenly():
    for pos, values in ((0, sorted(lp.FUSION_SOURCES)), (1, ("sum", "summax")), (2, (5, 19, 150, 300)), (3, (False, True))):
        for v in values:
            seen = [dealt(c) for c in FUSION_CASES if c[pos] == v]
            assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {0.0, 0.5, 1.0}, (pos, v)
            assert {s[2] for s in seen} == {"host", "device", "transposed"}, (pos, v)


@pytest.mark.parametrize("size,kind,C,with_map", FUSION_CASES)
def test_fuse_views_labels_bit_exact(sm, oracle, size, kind, C, with_map):
    """fuse_views_labels(resize="nearest", label_map=) on 11 views -- groups of 8 + 2 + 1 -- against the oracle fed one_hot of the
    reference-prepared masks: raw accumulator and get() equal in bits."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    with_weights, iew, how = dealt((size, kind, C, with_map))
    masks, m, planes = fusion_inputs(size, C, with_map, len(cams))
    rng = np.random.default_rng(9)
    weights = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) for _ in cams] if with_weights else None
    if how == "host":
        images, wts = masks, weights
    else:
        images = [to_device(x) if how == "device" else to_device(np.ascontiguousarray(x.T)).T for x in masks]
        wts = None if weights is None else [to_device(x) for x in weights]
    r = sm.render.triangles(mesh)
    agg = sm.fusion.MeshAggregator(P, C, kind, iew)
    before = option(sm, "labels_prepare_launches")
    agg.fuse_views_labels(r, cams, images, wts, resize="nearest", label_map=m)
    assert sm._lib.last_fuse_kernel() == NATIVE
    assert option(sm, "labels_prepare_launches") - before == len(cams)
    oagg = oracle.OracleAggregator(P, C, kind, iew)
    for k in range(len(cams)):
        oagg.add(oidx[k], one_hot(planes[k], C), None if weights is None else weights[k])
    got, want = agg.get_raw(), oagg.get_raw()
    assert bits(want).any()
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(agg.get()), bits(oagg.get()))


@pytest.mark.parametrize("C", [19, 300])
def test_big_triangles_take_the_tail_waves(sm, oracle, C):
    """A room of big triangles: queued triangles are summed by a wave, in tree order -- the float64-accumulating oracle at 1e-5."""
    from semantic_meshes_amd import synth
    rng = np.random.default_rng(40 + C)
    verts, faces, half = _room(rng, 8)
    cams = []
    for _ in range(5):
        R, t = synth.look_at(tuple(rng.uniform(-0.85, 0.85, 3) * half), tuple(rng.uniform(-1.0, 1.0, 3) * half), up=(0, 0, 1))
        f = float(rng.uniform(0.35, 1.2)) * W
        cams.append(sm.data.Camera(R, t, np.array([W, H]), np.array([f, f]), np.array([W / 2.0, H / 2.0])))
    mesh = types.SimpleNamespace(vertices=verts, faces=faces)
    P = len(faces)
    w, h = lp.FUSION_SOURCES["0.37"]
    m = lp.make_map(rng, 64, C)
    masks = [lp.make_source(rng, w, h, np.uint8, 64) for _ in cams]
    r = sm.render.triangles(mesh)
    o = oracle.OracleRenderer(verts, faces)
    agg = sm.fusion.MeshAggregator(P, C)
    agg.fuse_views_labels(r, cams, masks, resize="nearest", label_map=m)
    assert sm._lib.last_fuse_kernel() == NATIVE
    queued = 0
    for cam in cams:
        r.render(cam)
        queued += int(r.render_stats(cam, queues=True)[1][0])
    assert queued > 0
    oracle.set_accum_double(True)
    try:
        oagg = oracle.OracleAggregator(P, C)
        for cam, x in zip(cams, masks):
            oagg.add(o.render(cam)[0], one_hot(lp.prepare(x, C, (W, H), m), C))
        want, dist = oagg.get_raw(), oagg.get()
    finally:
        oracle.set_accum_double(False)
    assert_fused_close(agg.get_raw(), want)
    assert_fused_close(agg.get(), dist)


def test_fallback_routes_equal_the_plain_call_on_the_prepared_mask(sm, oracle):
    """Mul, a texel renderer and a foreign index image: with the keywords the result is, in bits, that of the plain call on the
    reference-prepared full-size mask, and the same kernel ran."""
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    cams = cams[:3]
    C = 19
    masks, m, planes = fusion_inputs("0.37", C, True, 11)
    r = sm.render.triangles(mesh)
    rt = sm.render.texels(mesh, cams, 0.05)

    def twin(renderer, prims, kind, foreign):
        a, b = sm.fusion.MeshAggregator(prims, C, kind), sm.fusion.MeshAggregator(prims, C, kind)
        kernels = []
        for k, cam in enumerate(cams):
            if foreign:
                idx = np.asarray(renderer.render(cam)[0]).copy()
                a.add_labels(idx, masks[k], resize="nearest", label_map=m)
                kernels.append(sm._lib.last_fuse_kernel())
                b.add_labels(idx, planes[k])
            else:
                a.fuse_view_labels(renderer, cam, masks[k], resize="nearest", label_map=m)
                kernels.append(sm._lib.last_fuse_kernel())
                b.fuse_view_labels(renderer, cam, planes[k])
            kernels.append(sm._lib.last_fuse_kernel())
        assert kernels[0::2] == kernels[1::2] and NATIVE not in kernels, kernels
        ra, rb = bits(a.get_raw()), bits(b.get_raw())
        assert rb.any()
        np.testing.assert_array_equal(ra, rb)

    twin(r, P, "mul", False)
    twin(rt, rt.getPrimitivesNum(), "sum", False)
    twin(r, P, "sum", True)
    a, b = sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C), sm.fusion.MeshAggregator(rt.getPrimitivesNum(), C)
    a.fuse_views_labels(rt, cams, masks[:3], resize="nearest", label_map=m)
    b.fuse_views_labels(rt, cams, planes[:3])
    np.testing.assert_array_equal(bits(a.get_raw()), bits(b.get_raw()))


def test_per_view_forms_keep_the_order_of_additions(sm, oracle):
    """add_labels / fuse_view_labels with the keywords between deferred plain add_labels calls: the bits of the same sequence issued
    eagerly (defer = False), and of the oracle."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    C = 19
    masks, m, planes = fusion_inputs("0.4", C, True, 11)
    r = sm.render.triangles(mesh)
    got = []
    for defer in (True, False):
        a = sm.fusion.MeshAggregator(P, C, "sum", 0.5)
        a.defer = defer
        pending = []
        for k in range(7):
            if k in (2, 5):
                a.add_labels(r.render(cams[k])[0], masks[k], resize="nearest", label_map=m)
            elif k == 3:
                a.fuse_view_labels(r, cams[k], to_device(masks[k]), resize="nearest", label_map=m)
            else:
                a.add_labels(r.render(cams[k])[0], to_device(planes[k]))
            pending.append(len(a._pending))
        assert (max(pending) > 0) == defer and pending[2] == pending[3] == pending[5] == 0
        got.append(bits(a.get_raw()))
    np.testing.assert_array_equal(got[0], got[1])
    oagg = oracle.OracleAggregator(P, C, "sum", 0.5)
    for k in range(7):
        oagg.add(oidx[k], one_hot(planes[k], C))
    np.testing.assert_array_equal(got[0], bits(oagg.get_raw()))


def test_equal_sizes_and_no_map_is_the_plain_call(sm, oracle):
    """resize="nearest" on a mask that has the view's size already: no prepare launch, the dense uint8 device plane is used in place
    and still joins a deferred group; the bits of the plain call."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    C = 19
    masks, m, planes = fusion_inputs("half", C, False, 11)
    d_planes = [to_device(p) for p in planes[:3]]
    r = sm.render.triangles(mesh)
    a, b = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    before = option(sm, "labels_prepare_launches")
    a.fuse_views_labels(r, cams[:3], d_planes, resize="nearest")
    a.add_labels(r.render(cams[3])[0], d_planes[0], resize="nearest")
    assert len(a._pending) == 1            # deferred like the plain call
    a.fuse_view_labels(r, cams[4], d_planes[1], resize="nearest")
    assert len(a._pending) == 2
    b.fuse_views_labels(r, cams[:3], d_planes)
    b.add_labels(r.render(cams[3])[0], d_planes[0])
    b.fuse_view_labels(r, cams[4], d_planes[1])
    ra, rb = bits(a.get_raw()), bits(b.get_raw())
    assert option(sm, "labels_prepare_launches") == before
    assert rb.any()
    np.testing.assert_array_equal(ra, rb)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3)])
def test_tiny_sources(sm, oracle, shape):
    """A (1,1) and a (2,3) mask into 160 x 120 views: the "at least 8 pixels" condition of the label kernel concerns the prepared
    plane, which is full size."""
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    C = 5
    rng = np.random.default_rng(shape[0])
    masks = [rng.integers(0, C, size=shape).astype(np.int64) for _ in range(3)]
    r = sm.render.triangles(mesh)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_views_labels(r, cams[:2], masks[:2], resize="nearest")
    a.add_labels(r.render(cams[2])[0], masks[2], resize="nearest")
    assert sm._lib.last_fuse_kernel() == NATIVE
    oagg = oracle.OracleAggregator(P, C)
    for k in range(3):
        oagg.add(oidx[k], one_hot(lp.prepare(masks[k], C, (W, H)), C))
    assert bits(oagg.get_raw()).any()
    np.testing.assert_array_equal(bits(a.get_raw()), bits(oagg.get_raw()))


# ---- ground truth ----------------------------------------------------------------------------------------------------------------
def test_ground_truth_with_a_map_and_at_another_size(sm, oracle):
    from semantic_meshes_amd.device import to_device
    from semantic_meshes_amd.evaluation import ConfusionMatrix
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    cams = cams[:3]
    C = 19
    masks, m, planes = fusion_inputs("0.37", C, True, 11)
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, C, size=P).astype(np.int32)
    r = sm.render.triangles(mesh)
    unmapped = [int((p[np.asarray(oidx[k]) < P] == 255).sum()) for k, p in enumerate(planes[:3])]
    assert min(unmapped) > 0

    def pair(with_keywords, plain):
        a, b = ConfusionMatrix(C), ConfusionMatrix(C)
        with_keywords(a)
        plain(b)
        Ma, Mb = a.get(), b.get()
        assert Mb.sum() > 0 and b.ignored > 0
        np.testing.assert_array_equal(Ma, Mb)
        assert a.ignored == b.ignored
        return a.ignored

    for images in (masks[:3], [to_device(x) for x in masks[:3]]):
        pair(lambda cm: cm.add_views(r, cams, labels, images, gt_resize="nearest", gt_map=m), lambda cm: cm.add_views(r, cams, labels, planes[:3]))
    pair(lambda cm: cm.add_view(r, cams[1], labels, masks[1], gt_resize="nearest", gt_map=m), lambda cm: cm.add_view(r, cams[1], labels, planes[1]))
    idx = np.asarray(r.render(cams[0])[0]).copy()
    pair(lambda cm: cm.add_image(idx, labels, masks[0], gt_resize="nearest", gt_map=m), lambda cm: cm.add_image(idx, labels, planes[0]))
    # add_probs: the ground truth defines the target size -- a map only
    full = lp.make_source(rng, W, H, np.uint16, 64)
    probs = rng.random((W, H, C), dtype=np.float32)
    pair(lambda cm: cm.add_probs(probs, full, gt_map=m), lambda cm: cm.add_probs(probs, lp.prepare(full, C, None, m)))
    pair(lambda cm: cm.add_probs_many([probs], [to_device(full)], gt_map=m), lambda cm: cm.add_probs_many([probs], [lp.prepare(full, C, None, m)]))
    # 1-D
    pred, gt = rng.integers(-1, C, size=501).astype(np.int32), lp.make_source(rng, 501, 1, np.int32, 64)[:, 0]
    pair(lambda cm: cm.add(pred, gt, gt_map=m), lambda cm: cm.add(pred, lp.prepare(gt.reshape(-1, 1), C, None, m)[:, 0]))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(sm, oracle):
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    C = 19
    masks, m, planes = fusion_inputs("0.37", C, True, 11)
    r = sm.render.triangles(mesh)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view_labels(r, cams[0], masks[0], resize="nearest", label_map=m)
    before = bits(a.get_raw()).copy()
    assert before.any()
    a.add_labels(r.render(cams[1])[0], to_device(planes[1]))      # one deferred view: a refused call must leave it pending
    assert len(a._pending) == 1
    small = masks[2]
    python_calls = [lambda: a.add_labels(r.render(cams[2])[0], small), lambda: a.add_labels(r.render(cams[2])[0], small, resize="bilinear"),
                    lambda: a.add_labels(r.render(cams[2])[0], small, label_map=m), lambda: a.fuse_view_labels(r, cams[2], small),
                    lambda: a.fuse_view_labels(r, cams[2], small, resize="nearest", label_map=np.zeros(0, np.int32)),
                    lambda: a.fuse_views_labels(r, cams[2:4], [small, small], label_map=m.astype(np.float32)),
                    lambda: a.fuse_views_labels(r, cams[2:4], [small, np.zeros((0, 4), np.int32)], resize="nearest"),
                    lambda: a.fuse_views_labels(r, cams[2:4], [small, small.astype(np.float32)], resize="nearest")]
    for call in python_calls:
        with pytest.raises(ValueError):
            call()
        assert len(a._pending) == 1
    # the C entry points
    lib, chk = sm._lib.lib(), sm._lib.check
    w, h = small.shape
    pod, lptr = ctypes.byref(cams[2]._pod), small.ctypes.data_as(ctypes.c_void_p)
    mptr = m.ctypes.data_as(ctypes.c_void_p)
    i32, host = sm._lib.LBL_CODES["int32"], sm._lib.MEM_HOST
    handle = a._handle

    def fuse(dtype=i32, strides=None, mem=host, w=w, h=h, mp=mptr, mlen=len(m), mmem=host):
        return lib.smesh_fuse_view_labels_prepared(r._h, handle, pod, lptr, dtype, strides, None, mem, w, h, mp, mlen, mmem)

    for kw in (dict(w=0), dict(h=0), dict(w=65537), dict(mlen=0), dict(mlen=(1 << 24) + 1), dict(mp=None), dict(dtype=8), dict(dtype=-1),
               dict(mem=2), dict(mmem=5), dict(strides=(ctypes.c_int64 * 2)(-1, 1))):
        assert fuse(**kw) == sm._lib.ERR_INVALID, kw
        assert sm._lib.lib().smesh_last_error()
    idx = np.asarray(oidx[2]).astype(np.uint32)
    assert lib.smesh_aggregator_add_labels_prepared(handle, None, idx.ctypes.data_as(ctypes.c_void_p), sm._lib.IDX_U32, None, host, lptr, i32, None, host,
                                                    None, None, host, W, H, 0, h, mptr, len(m), host) == sm._lib.ERR_INVALID
    from semantic_meshes_amd.device import DeviceBuffer
    out = DeviceBuffer(W * H * 2, 0)
    for args in ((0, h, None, 0, host, C, 0), (w, h, mptr, 0, host, C, 0), (w, h, None, 0, host, 300, 0), (w, h, None, 0, host, 70000, 2),
                 (w, h, None, 0, host, C, 5)):
        sw, sh, mp, mlen, mmem, classes, odt = args
        assert lib.smesh_labels_prepare(lptr, i32, None, host, sw, sh, mp, mlen, mmem, classes, ctypes.c_void_p(out.ptr), odt, W, H, 0) == sm._lib.ERR_INVALID, args
    assert len(a._pending) == 1
    with a._pending_lock:
        a._pending = []          # drop the deferred view: what is left must be the bits from before the refused calls
    np.testing.assert_array_equal(bits(a.get_raw()), before)
    chk(lib.smesh_synchronize(0))
