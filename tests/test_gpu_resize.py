"""Class-vector images resampled from the network's resolution to the camera's, on the GPU (include/smesh_resize.h): every entry point
against resize_ref.py -- the numpy restatement of DESIGN.md 3.8 -- on the exactly widened image, bit for bit.  Labels are
probs_labels_ref.ref_labels of the resampled float32 image; fusion is the CPU oracle fed the resampled images."""
import ctypes
import os

import numpy as np
import pytest

import half_helpers as hh
import probs_labels_ref as pl
import resize_ref as ref
from helpers import assert_fused_close, random_probs
from test_gpu_half import NATIVE, check_against_oracle, oracle_raw, scene
from test_gpu_labels import bits, expected_launches, fuse_slot_counts

pytestmark = pytest.mark.gpu

CLASSES = (1, 3, 4, 5, 8, 19, 40, 41, 150)           # no vector piece, pieces of four and eight, a tail, the workloads' counts, many
THREE_SHAPES = (((4, 3), (8, 6)), ((13, 9), (5, 4)), ((37, 53), (130, 67)))
TWO_SHAPES = (((5, 4), (13, 9)), ((40, 30), (81, 61)))
_cache = {}


def shape_id(shape):
    return "%dx%d-%dx%d" % (shape[0] + shape[1])


@pytest.fixture(params=[1, 0], ids=["vector", "generic"])
def vector(sm, request):
    before = sm._lib.get_option("resize_vector")
    sm._lib.set_option("resize_vector", request.param)
    yield request.param
    sm._lib.set_option("resize_vector", before)


def source(w, h, C, dtype, special=False):
    """(values, widened) of one seeded source image, generated once and left unchanged."""
    key = ("src", w, h, C, dtype, special)
    if key not in _cache:
        rng = np.random.default_rng(w * 100003 + h * 1009 + C * 7 + ref.DTYPES.index(dtype))
        _cache[key] = ref.make_source(rng, w, h, C, dtype, special)
    return _cache[key]


def resized(w, h, C, dtype, W, H):
    """ref_resize of that image, computed once."""
    key = ("ref", w, h, C, dtype, W, H)
    if key not in _cache:
        _cache[key] = ref.ref_resize(source(w, h, C, dtype)[1], W, H)
    return _cache[key]


def got_bits(out, out_dtype):
    """The library's (W,H,C) result as comparable bits: float32 values, or the uint16 patterns of a 16-bit image."""
    a = np.asarray(out)
    return a if out_dtype == "float32" else a.view(np.uint16)


def want_bits(wide_resized, out_dtype):
    return wide_resized if out_dtype == "float32" else hh.narrow(wide_resized, out_dtype)


# ---- 1. smesh_resize_probs / resize_probs_device ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_dense_float32_at_every_shape_and_class_count(sm, vector, shape):
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = shape
    for C in CLASSES:
        values, wide = source(w, h, C, "float32")
        out = sm.fusion.resize_probs_device(to_device(values), (W, H))
        assert type(out).__name__ == "DeviceArray" and out.shape == (W, H, C) and out.dtype == np.float32
        assert out.strides == (H * C, C, 1) and not out.bfloat16
        assert np.array_equal(np.asarray(out), resized(w, h, C, "float32", W, H)), C


@pytest.mark.parametrize("out_dtype", ref.DTYPES)
@pytest.mark.parametrize("in_dtype", ref.DTYPES)
def test_all_nine_dtype_pairs(sm, vector, in_dtype, out_dtype):
    from semantic_meshes_amd.device import to_device
    for (w, h), (W, H) in THREE_SHAPES:
        for C in (8, 19):
            values, wide = source(w, h, C, in_dtype)
            out = sm.fusion.resize_probs_device(to_device(values), (W, H), out_dtype=out_dtype, **hh.kw(in_dtype))
            assert out.dtype == {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[out_dtype]
            assert out.bfloat16 == (out_dtype == "bfloat16")
            want = want_bits(resized(w, h, C, in_dtype, W, H), out_dtype)
            assert np.array_equal(got_bits(out, out_dtype), want), (w, h, W, H, C)
            if in_dtype == out_dtype:      # the default out_dtype is the input's
                same = sm.fusion.resize_probs(to_device(values), (W, H), **hh.kw(in_dtype))
                assert np.array_equal(got_bits(same, out_dtype), want)


def layouts(sm, values, dtype):
    """[(name, device array, host array)]: one (w,h,C) image in the layouts a caller may hand over."""
    from semantic_meshes_amd.device import DeviceArray, to_device
    w, h, C = values.shape

    def mark(d):
        d.bfloat16 = dtype == "bfloat16"
        return d

    out = [("dense", mark(to_device(values)), values)]
    hwc = np.ascontiguousarray(values.transpose(1, 0, 2))                      # a network's (h,w,C) tensor ...
    out.append(("hwc", mark(to_device(hwc).transpose(1, 0, 2)), hwc.transpose(1, 0, 2)))     # ... seen as (w,h,C): strides (C, w C, 1)
    chw = np.ascontiguousarray(values.transpose(2, 1, 0))                      # channel-first (C,h,w) ...
    out.append(("chw", mark(to_device(chw).transpose(2, 1, 0)), chw.transpose(2, 1, 0)))     # ... seen as (w,h,C): strides (1, w, h w)
    flat = np.concatenate([values.reshape(-1)[:1], values.reshape(-1)])       # one element into a flat buffer: element alignment only
    buf = to_device(flat)
    out.append(("offset", mark(DeviceArray(buf.ptr + values.itemsize, (w, h, C), values.dtype, 0, owner=buf)), None))
    wide2 = np.zeros((w, h, 2 * C), values.dtype)
    wide2[:, :, ::2] = values
    wide2[:, :, 1::2] = values[:, :, ::-1]                                      # (what a kernel that ignored the class stride would read)
    buf2 = to_device(wide2)
    out.append(("class-stride-2", mark(DeviceArray(buf2.ptr, (w, h, C), values.dtype, 0, strides=(h * 2 * C, 2 * C, 2), owner=buf2)),
                wide2[:, :, ::2]))
    return out


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_layouts_and_host_images(sm, vector, dtype):
    for (w, h), (W, H) in TWO_SHAPES:
        for C in (8, 19):
            values, wide = source(w, h, C, dtype)
            want = want_bits(resized(w, h, C, dtype, W, H), dtype)
            for name, dev, host in layouts(sm, values, dtype):
                assert dev.shape == (w, h, C)
                out = sm.fusion.resize_probs_device(dev, (W, H), **hh.kw(dtype))
                assert out.shape == (W, H, C) and out.strides == (H * C, C, 1)
                assert np.array_equal(got_bits(out, dtype), want), (name, w, h, C)
                if host is not None:          # a host image gives what the device image gives
                    assert host.shape == (w, h, C)
                    assert np.array_equal(got_bits(sm.fusion.resize_probs(host, (W, H), **hh.kw(dtype)), dtype), want), (name, "host", w, h, C)


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_identity_size_is_an_exact_copy_with_nan_and_infinities(sm, vector, dtype):
    from semantic_meshes_amd.device import to_device
    w, h = 7, 5
    for C in (5, 8):
        values, wide = source(w, h, C, dtype, special=True)
        assert np.isnan(wide).any() and np.isposinf(wide).any() and np.isneginf(wide).any()
        out = sm.fusion.resize_probs(to_device(values), (w, h), **hh.kw(dtype))
        got = ref.widened(out, dtype)
        assert np.array_equal(got, wide, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(wide))
        if dtype == "float32":
            assert np.array_equal(got.view(np.uint32), wide.view(np.uint32))      # (float32: the NaN's bits too)


def test_the_c_entry_point_refuses_and_touches_nothing(sm):
    from semantic_meshes_amd.device import to_device
    L, lib = sm._lib, sm._lib.lib()
    w, h, C, W, H = 4, 3, 8, 8, 6
    src = to_device(source(w, h, C, "float32")[0])
    out = to_device(np.full((W, H, C), 7.0, np.float32))
    p, o = ctypes.c_void_p(src.ptr), ctypes.c_void_p(out.ptr)

    def call(**k):
        a = dict(inp=p, idt=L.PROBS_F32, istr=None, mem=L.MEM_DEVICE, w=w, h=h, C=C, out=o, odt=L.PROBS_F32, W=W, H=H, mode=L.RESIZE_BILINEAR)
        a.update(k)
        return lib.smesh_resize_probs(a["inp"], a["idt"], a["istr"], a["mem"], a["w"], a["h"], a["C"], a["out"], a["odt"], a["W"], a["H"], a["mode"], 0)

    neg = (ctypes.c_int64 * 3)(h * C, -C, 1)
    for k in (dict(mode=0), dict(mode=2), dict(idt=3), dict(odt=-1), dict(C=0), dict(w=0), dict(h=0), dict(W=65537), dict(mem=2),
              dict(istr=neg), dict(inp=None), dict(out=None), dict(out=p, W=w, H=h),                      # out is in
              dict(out=ctypes.c_void_p(src.ptr + 16), W=2, H=1)):                                         # out overlaps in
        assert call(**k) == L.ERR_INVALID and lib.smesh_last_error(), k
    assert call(W=0) == L.OK and call(H=0) == L.OK and call(W=0, w=0) == L.OK       # nothing to do
    sm._lib.synchronize(0)
    assert (np.asarray(out) == 7.0).all()
    assert call() == L.OK
    assert np.array_equal(np.asarray(out), resized(w, h, C, "float32", W, H))


# ---- 2. smesh_resize_probs_labels -----------------------------------------------------------------------------------------------
def label_source(w, h, C, dtype):
    """(values, widened) for the label tests: softmax rows with the planted rows of probs_labels_ref (NaN, infinities, ties within a
    row), and -- from three classes on -- the left half of the image with twice its row maximum at classes C // 3 AND C - 1: every
    corner of a pixel there is tied, the blend of tied values is tied, and the lower class must win."""
    key = ("lsrc", w, h, C, dtype)
    if key not in _cache:
        rng = np.random.default_rng(w * 7919 + h * 104729 + C * 31 + ref.DTYPES.index(dtype))
        _, wide, _ = pl.make_probs(rng, w, h, C, dtype)
        wide = wide.copy()
        if C >= 3:
            half = max(w // 2, 1)
            with np.errstate(invalid="ignore"):
                m = np.fmax.reduce(wide[:half], axis=-1)
            m = np.where(np.isnan(m), np.float32(0.5), np.float32(2.0) * m)       # (a power of two: exact in every dtype)
            wide[:half, :, C // 3] = m
            wide[:half, :, C - 1] = m
        if dtype == "float32":
            values = wide
        else:
            b = hh.narrow(wide, dtype)
            assert np.array_equal(hh.widen(b, dtype), wide, equal_nan=True)      # (every planted value was an element already)
            values = hh.typed(b, dtype)
        _cache[key] = (values, wide)
    return _cache[key]


def label_reference(w, h, C, dtype, W, H, thr):
    key = ("lref", w, h, C, dtype, W, H, thr)
    if key not in _cache:
        big = ref.ref_resize(label_source(w, h, C, dtype)[1], W, H)
        _cache[key] = pl.ref_labels(big, thr)
    return _cache[key]


@pytest.mark.parametrize("thr", [None, 0.9])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_labels_of_the_resampled_image(sm, vector, dtype, thr):
    from semantic_meshes_amd.device import to_device
    for (w, h), (W, H) in (((1, 1), (6, 5)), ((5, 4), (13, 9)), ((13, 9), (5, 4)), ((37, 53), (130, 67))):
        for C in (1, 2, 19, 40, 150, 300):
            values, wide = label_source(w, h, C, dtype)
            lab, dc = label_reference(w, h, C, dtype, W, H, thr)
            if C >= 3 and w >= 4:
                x1 = ref.axis_table(w, W)[1]
                tied = x1 < max(w // 2, 1)                    # output columns all of whose corners lie in the tied half
                assert tied.any() and (lab[tied] != C - 1).all() and (w < 13 or (lab[tied] == C // 3).mean() > 0.5)
            if thr is not None and C > 1 and W * H > 30:
                assert dc.any() and not dc.all()
            for out_dt in (np.uint8, np.uint16, np.int32):
                if C > np.iinfo(out_dt).max:
                    with pytest.raises(ValueError):
                        sm.fusion.argmax_labels(to_device(values), thr, dtype=out_dt, size=(W, H), resize="bilinear", **hh.kw(dtype))
                    continue
                got = sm.fusion.argmax_labels_device(to_device(values), thr, dtype=out_dt, size=(W, H), resize="bilinear", **hh.kw(dtype))
                assert got.shape == (W, H) and got.dtype == out_dt and got.strides == (H, 1)
                want = np.where(dc, np.iinfo(out_dt).max, lab).astype(out_dt)
                assert np.array_equal(np.asarray(got), want), (w, h, W, H, C, out_dt)
            host = sm.fusion.argmax_labels(values, thr, dont_care_label=-1, dtype=np.int32, size=(W, H), resize="bilinear", **hh.kw(dtype))
            assert np.array_equal(host, np.where(dc, -1, lab).astype(np.int32)), (w, h, W, H, C, "host")


def test_labels_into_a_strided_image_and_from_permuted_views(sm, vector):
    from semantic_meshes_amd.device import to_device
    L, lib = sm._lib, sm._lib.lib()
    (w, h), (W, H), C = (40, 30), (81, 61), 19
    for dtype in ref.DTYPES:
        values, wide = label_source(w, h, C, dtype)
        lab, dc = label_reference(w, h, C, dtype, W, H, 0.9)
        want = np.where(dc, 255, lab).astype(np.uint8)
        for name, dev, host in layouts(sm, values, dtype):
            assert np.array_equal(sm.fusion.argmax_labels(dev, 0.9, size=(W, H), resize="bilinear", **hh.kw(dtype)), want), (dtype, name)
        # a strided output through the C entry point: x stride 2 H + 3, y stride 2; everything between stays as it was
        s0, s1 = 2 * H + 3, 2
        canvas = to_device(np.full(W * s0, 200, np.uint8))
        src = to_device(values)
        code = {"float32": L.PROBS_F32, "float16": L.PROBS_F16, "bfloat16": L.PROBS_BF16}[dtype]
        L.check(lib.smesh_resize_probs_labels(ctypes.c_void_p(src.ptr), code, None, L.MEM_DEVICE, w, h, C, 0.9, ctypes.c_void_p(canvas.ptr),
                                              L.LBL_CODES["uint8"], (ctypes.c_int64 * 2)(s0, s1), 255,
                                              W, H, L.RESIZE_BILINEAR, 0))
        flat = np.asarray(canvas)
        picked = np.lib.stride_tricks.as_strided(flat, (W, H), (s0, s1))
        assert np.array_equal(picked, want), dtype
        mask = np.ones(W * s0, bool)
        np.lib.stride_tricks.as_strided(mask, (W, H), (s0, s1))[...] = False
        assert (flat[mask] == 200).all()


# ---- 3. ConfusionMatrix.add_probs(..., resize="bilinear") ------------------------------------------------------------------------
@pytest.mark.parametrize("C", [19, 63, 64, 150])
def test_add_probs_resized_counts_the_reference_labels(sm, vector, C):
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = (37, 53), (130, 67)
    rng = np.random.default_rng(C)
    for k, dtype in enumerate(ref.DTYPES):
        values, wide = label_source(w, h, C, dtype)
        thr = (None, 0.9, 0.9)[k]
        lab, dc = label_reference(w, h, C, dtype, W, H, thr)
        pred = np.where(dc, -1, lab)
        g8, g32 = pl.make_gt(rng, (W, H), C, "uint8"), pl.make_gt(rng, (W, H), C, "int32")
        ghw = np.ascontiguousarray(pl.make_gt(rng, (W, H), C, "uint8").T)            # decoded as (H,W), passed as its transposed view
        cases = [("uint8 host", g8, g8), ("int32 host", g32, g32), ("uint8 device", to_device(g8), g8), ("(H,W) transposed", ghw.T, ghw.T)]
        cm = sm.fusion.ConfusionMatrix(C)
        want, ignored = np.zeros((C, C + 1), np.uint64), 0
        for name, gt, gt_host in cases:
            dev = to_device(values) if "device" in name else values
            assert cm.add_probs(dev, gt, thr, resize="bilinear", **hh.kw(dtype)) is None
            M, ign = pl.expected_matrix(pred, gt_host, C)
            want, ignored = want + M, ignored + ign
            assert np.array_equal(cm.get(), want) and cm.ignored == ignored, (dtype, name)
        # labels_out=True: the label image of that pass
        out = cm.add_probs(to_device(values), g8, thr, labels_out=True, resize="bilinear", **hh.kw(dtype))
        dt = np.uint8 if C <= 255 else np.uint16
        assert out.shape == (W, H) and out.dtype == dt
        assert np.array_equal(np.asarray(out), np.where(dc, np.iinfo(dt).max, lab).astype(dt))
        M, ign = pl.expected_matrix(pred, g8, C)
        want, ignored = want + M, ignored + ign
        # equal sizes with the keyword: the image is scored as it is
        big = want_bits(ref.ref_resize(wide, W, H), dtype)
        big_wide = big if dtype == "float32" else hh.widen(big, dtype)
        cm.add_probs_many([hh.typed(big, dtype) if dtype != "float32" else big], [g8], thr, resize="bilinear", **hh.kw(dtype))
        l2, d2 = pl.ref_labels(big_wide, thr)
        M, ign = pl.expected_matrix(np.where(d2, -1, l2), g8, C)
        want, ignored = want + M, ignored + ign
        assert np.array_equal(cm.get(), want) and cm.ignored == ignored, dtype
        # a refused call leaves the matrix unchanged
        L, lib = sm._lib, sm._lib.lib()
        src, gd = to_device(values), to_device(g8)
        code = {"float32": L.PROBS_F32, "float16": L.PROBS_F16, "bfloat16": L.PROBS_BF16}[dtype]
        for mode, gdt, ww in ((0, L.LBL_CODES["uint8"], w), (L.RESIZE_BILINEAR, 99, w), (L.RESIZE_BILINEAR, L.LBL_CODES["uint8"], 0)):
            status = lib.smesh_confusion_add_probs_resized(cm._h, ctypes.c_void_p(src.ptr), code, None, L.MEM_DEVICE, ww, h,
                                                           ctypes.c_void_p(gd.ptr), gdt, None, L.MEM_DEVICE, W, H, float("-inf"), mode,
                                                           None, 0, None, 0)
            assert status == L.ERR_INVALID and lib.smesh_last_error()
        with pytest.raises(ValueError):
            cm.add_probs(values, g8[:, :-1].astype(np.float32), resize="bilinear", **hh.kw(dtype))
        with pytest.raises(ValueError, match="ground truth must have shape"):
            cm.add_probs(values, g8, **hh.kw(dtype))                                 # without the keyword: as before
        assert np.array_equal(cm.get(), want) and cm.ignored == ignored


# ---- 4. fusion --------------------------------------------------------------------------------------------------------------------
W, H = 160, 120                      # test_gpu_half's scenes
SOURCES = {"half": (80, 60), "0.37": (59, 44)}


def fusion_images(C, dtype, size, n, positive=False):
    """`n` source images (values, widened) at `size`, and what the fusion must see: ref_resize of each, rounded to the input's dtype
    (the resampled array has the input's dtype) and widened again."""
    key = ("fimg", C, dtype, size, n, positive)
    if key not in _cache:
        w, h = size
        rng = np.random.default_rng(1000 * C + 13 * w + ref.DTYPES.index(dtype))
        small, big = [], []
        for _ in range(n):
            if dtype == "float32":
                p = random_probs(rng, w, h, C)
                if positive:
                    p = np.maximum(p, np.float32(1e-3))
                values = wide = p
            else:
                b = hh.random_probs16(rng, w, h, C, dtype)
                values, wide = hh.typed(b, dtype), hh.widen(b, dtype)
            small.append((values, wide))
            r = ref.ref_resize(wide, W, H)
            big.append(r if dtype == "float32" else hh.widen(hh.narrow(r, dtype), dtype))
        _cache[key] = (small, big)
    return _cache[key]


def marked(sm, values, dtype):
    from semantic_meshes_amd.device import to_device
    d = to_device(values)
    d.bfloat16 = dtype == "bfloat16"
    return d


@pytest.mark.parametrize("size", sorted(SOURCES))
@pytest.mark.parametrize("C", [19, 40])
@pytest.mark.parametrize("kind", ["sum", "summax"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_fuse_views_resized_against_the_library_and_the_oracle(sm, oracle, dtype, kind, C, size):
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")      # no queued triangles: one lane owns a row, the oracle's bits
    assert sum(queued) == 0
    P, n = len(mesh.faces), len(cams)
    small, big = fusion_images(C, dtype, SOURCES[size], n)
    iew = [0.0, 0.5, 1.0][(C + len(kind)) % 3]
    a = sm.fusion.MeshAggregator(P, C, kind, iew)
    a.fuse_views(r, cams, [marked(sm, v, dtype) for v, _ in small], resize="bilinear")
    if dtype == "float16":
        assert sm._lib.last_fuse_kernel() == NATIVE
    got = check_against_oracle(oracle, a, P, C, kind, iew, oidx, big, sum(queued))
    b = sm.fusion.MeshAggregator(P, C, kind, iew)
    pre = [sm.fusion.resize_probs_device(marked(sm, v, dtype), (W, H)) for v, _ in small]
    assert all(p.dtype == small[0][0].dtype and p.shape == (W, H, C) for p in pre)
    b.fuse_views(r, cams, pre)
    np.testing.assert_array_equal(bits(b.get_raw()), bits(got))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_fuse_views_resized_on_the_coarse_scene(sm, oracle, dtype):
    """helpers.small_scene() as it is: triangles of up to 15 pixels are queued and summed in tree order, so the reference is the
    float64-accumulating oracle (check_against_oracle), and the two routes through the library agree within the same bound."""
    C, kind = 19, "sum"
    mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
    P, n = len(mesh.faces), len(cams)
    small, big = fusion_images(C, dtype, SOURCES["0.37"], n)
    a = sm.fusion.MeshAggregator(P, C, kind)
    a.fuse_views(r, cams, [marked(sm, v, dtype) for v, _ in small], resize="bilinear")
    got = check_against_oracle(oracle, a, P, C, kind, 0.5, oidx, big, sum(queued))
    b = sm.fusion.MeshAggregator(P, C, kind)
    b.fuse_views(r, cams, [sm.fusion.resize_probs_device(marked(sm, v, dtype), (W, H)) for v, _ in small])
    if sum(queued) == 0:
        np.testing.assert_array_equal(bits(b.get_raw()), bits(got))
    else:
        assert_fused_close(b.get_raw(), got)


def test_fuse_views_resized_mul(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = fusion_images(C, "float32", SOURCES["0.37"], 4, positive=True)
    agg = sm.fusion.MeshAggregator(P, C, "mul")
    agg.fuse_views(r, cams[:4], [marked(sm, v, "float32") for v, _ in small], resize="bilinear")
    want = oracle_raw(oracle, P, C, "mul", 0.5, oidx[:4], big, double=True)[1]
    assert_fused_close(agg.get(), want, rtol=1e-5, atol=1e-6)


def test_render_add_loop_resized_is_one_eight_view_launch(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    for dtype in ("float32", "bfloat16"):
        small, big = fusion_images(C, dtype, SOURCES["half"], 8)
        dev = [marked(sm, v, dtype) for v, _ in small]
        agg = sm.fusion.MeshAggregator(P, C)
        assert agg.defer

        def loop():
            for k in range(8):
                idx, depth = r.render(cams[k])
                agg.add(idx, dev[k], resize="bilinear")
                assert idx.unrun and len(agg._pending) == (k + 1) % 8
        launches, fused = fuse_slot_counts(sm, loop)
        cap = max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8")))
        assert (launches, fused) == (expected_launches(8, cap), 8)            # one launch of eight views
        assert sm._lib.last_fuse_kernel() == (NATIVE if dtype == "bfloat16" else "k_fuse_tri")
        check_against_oracle(oracle, agg, P, C, "sum", 0.5, oidx[:8], big, 0)


def test_add_many_fuse_view_and_host_images_resized(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = fusion_images(C, "float16", SOURCES["0.37"], 11)
    agg = sm.fusion.MeshAggregator(P, C, "summax")
    planes = [r.render(cam)[0] for cam in cams[:11]]
    agg.add_many(planes, [marked(sm, v, "float16") for v, _ in small], resize="bilinear")
    want = check_against_oracle(oracle, agg, P, C, "summax", 0.5, oidx[:11], big, 0)
    one = sm.fusion.MeshAggregator(P, C, "summax")
    for k in range(11):
        one.fuse_view(r, cams[k], marked(sm, small[k][0], "float16"), resize="bilinear")
    np.testing.assert_array_equal(bits(one.get_raw()), bits(want))
    host = sm.fusion.MeshAggregator(P, C, "summax")                   # numpy images at the source's size: eleven views, two chunks
    host.fuse_views(r, cams[:11], [v for v, _ in small], resize="bilinear")
    np.testing.assert_array_equal(bits(host.get_raw()), bits(want))
    # equal sizes with the keyword: passed through untouched
    full = sm.fusion.MeshAggregator(P, C, "summax")
    full.fuse_views(r, cams[:11], [marked(sm, hh.typed(hh.narrow(b, "float16"), "float16"), "float16") for b in big], resize="bilinear")
    np.testing.assert_array_equal(bits(full.get_raw()), bits(want))


def test_a_refused_call_leaves_the_aggregator_unchanged(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = fusion_images(C, "float32", SOURCES["half"], 8)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view(r, cams[0], marked(sm, small[0][0], "float32"), resize="bilinear")
    before = bits(a.get_raw()).copy()
    assert before.any()
    good, wrong = marked(sm, small[1][0], "float32"), marked(sm, np.ascontiguousarray(small[1][0][:, :, :-1]), "float32")
    for bad, kwargs in ((wrong, {"resize": "bilinear"}), (good, {"resize": "nearest"}), (good, {}),
                        (marked(sm, small[1][0].astype(np.float64), "float32"), {"resize": "bilinear"})):
        with pytest.raises(ValueError):
            a.add(r.render(cams[1])[0], bad, **kwargs)
        with pytest.raises(ValueError):
            a.add_many([r.render(cams[1])[0]], [bad], **kwargs)
        with pytest.raises(ValueError):
            a.fuse_view(r, cams[1], bad, **kwargs)
        with pytest.raises(ValueError):
            a.fuse_views(r, [cams[1]], [bad], **kwargs)
    assert not a._pending
    np.testing.assert_array_equal(bits(a.get_raw()), before)
