"""(w,h,C) class vectors sampled inside the fusion kernel (include/smesh_sampled.h, `sample_in_kernel=True`): every entry point against
the resample-then-fuse route of `resize="bilinear"` and against the CPU oracle fed resize_ref.ref_resize of the widened source,
rounded to the source's dtype and widened again.  Bit for bit where one lane owns a row (the "fine" scene); within
helpers.assert_fused_close of the float64-accumulating oracle where triangles are queued and summed in tree order."""
import ctypes
import os

import numpy as np
import pytest

import half_helpers as hh
import sampled_inputs as si
import resize_ref as ref
from helpers import assert_fused_close, random_probs
from test_gpu_half import NATIVE, check_against_oracle, oracle_raw, scene
from test_gpu_labels import bits, expected_launches, fuse_slot_counts
from test_gpu_resize import marked

pytestmark = pytest.mark.gpu

SAMPLED = "k_fuse_tri_sampled"
W, H = si.W, si.H
KW = {"resize": "bilinear", "sample_in_kernel": True}


def cap():
    return max(1, int(os.environ.get("SMESH_FUSE_VIEWS", "8")))


def device(sm, small, dtype):
    return [marked(sm, v, dtype) for v, _ in small]


def instance(sm):
    return sm._lib.get_option("last_fuse_slot"), sm._lib.get_option("last_fuse_views")


# ---- 1. the main path, bit-exact ---------------------------------------------------------------------------------------------------
MAIN_CASES = si.main_cases()        # iew 0, 0.5 and 1 each with every (dtype, kind) pair, both class counts and every source size
assert {c[4] for c in MAIN_CASES} == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("dtype,kind,C,size,iew", MAIN_CASES)
def test_fuse_views_sampled_against_the_resampling_route_and_the_oracle(sm, oracle, dtype, kind, C, size, iew):
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")      # no queued triangles: one lane owns a row, the oracle's bits
    assert sum(queued) == 0
    P, n = len(mesh.faces), 11                                   # launches of 8 + 2 + 1 views
    small, big = si.source_images(C, dtype, si.SOURCES[size], 15)
    a = sm.fusion.MeshAggregator(P, C, kind, iew)
    dev = device(sm, small[:n], dtype)
    launches, fused = fuse_slot_counts(sm, lambda: a.fuse_views(r, cams[:n], dev, **KW))
    assert sm._lib.last_fuse_kernel() == SAMPLED
    assert instance(sm) == ((C + 7) // 8 * 8, 1)                  # the last launch of 8 + 2 + 1
    assert (launches, fused) == (expected_launches(n, cap()), n)
    got = check_against_oracle(oracle, a, P, C, kind, iew, oidx[:n], big[:n], 0)
    b = sm.fusion.MeshAggregator(P, C, kind, iew)
    b.fuse_views(r, cams[:n], device(sm, small[:n], dtype), resize="bilinear")
    assert sm._lib.last_fuse_kernel() in ("k_fuse_tri", NATIVE)
    np.testing.assert_array_equal(bits(b.get_raw()), bits(got))


@pytest.mark.parametrize("dtype", si.DTYPES)
def test_fifteen_views_are_four_launches(sm, oracle, dtype):
    C, kind, iew = 19, "sum", 0.5
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], 15)
    a = sm.fusion.MeshAggregator(P, C, kind, iew)
    dev = device(sm, small, dtype)
    launches, fused = fuse_slot_counts(sm, lambda: a.fuse_views(r, cams, dev, **KW))
    assert sm._lib.last_fuse_kernel() == SAMPLED
    assert (launches, fused) == (expected_launches(15, cap()), 15)           # 8 + 4 + 2 + 1 views
    check_against_oracle(oracle, a, P, C, kind, iew, oidx, big, 0)


# ---- 2. slot edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", si.DTYPES)
@pytest.mark.parametrize("C", [1, 8, 9, 16, 17, 19, 24, 25, 32, 33, 40, 41, 48, 49])
def test_every_slot_edge(sm, oracle, C, dtype):
    """The class counts around every register-slot boundary: where a tail piece of a row load can go wrong.  49 classes fall back."""
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P, n = len(mesh.faces), 3
    kind = "summax" if C % 2 else "sum"
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], n)
    a = sm.fusion.MeshAggregator(P, C, kind)
    a.fuse_views(r, cams[:n], device(sm, small, dtype), **KW)
    if C <= 48:
        assert sm._lib.last_fuse_kernel() == SAMPLED and sm._lib.get_option("last_fuse_slot") == (C + 7) // 8 * 8
    else:
        assert sm._lib.last_fuse_kernel() != SAMPLED
    got = a.get_raw()
    if C <= 48:
        check_against_oracle(oracle, a, P, C, kind, 0.5, oidx[:n], big, 0)
    b = sm.fusion.MeshAggregator(P, C, kind)
    b.fuse_views(r, cams[:n], device(sm, small, dtype), resize="bilinear")
    assert np.abs(got).sum() > 0
    np.testing.assert_array_equal(bits(b.get_raw()), bits(got))


# ---- 3. layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", si.DTYPES)
@pytest.mark.parametrize("C", [19, 40])
def test_layouts(sm, oracle, C, dtype):
    from semantic_meshes_amd.device import DeviceArray, to_device
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P, n = len(mesh.faces), 3
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], n)
    w, h = si.SOURCES["0.37"]
    want = oracle_raw(oracle, P, C, "sum", 0.5, oidx[:n], big)[0]

    def mark(d):
        d.bfloat16 = dtype == "bfloat16"
        return d

    def fused(images, kernel_is_sampled):
        a = sm.fusion.MeshAggregator(P, C)
        a.fuse_views(r, cams[:n], images, **KW, **(hh.kw(dtype) if isinstance(images[0], np.ndarray) else {}))
        assert (sm._lib.last_fuse_kernel() == SAMPLED) == kernel_is_sampled
        np.testing.assert_array_equal(bits(a.get_raw()), bits(want))

    # a network's (h,w,C) tensor seen as (w,h,C): strides (C, w C, 1), read in place
    fused([mark(to_device(np.ascontiguousarray(v.transpose(1, 0, 2))).transpose(1, 0, 2)) for v, _ in small], True)
    # a channel-first (C,h,w) tensor seen as (w,h,C): class stride h w -- resampled, then fused
    fused([mark(to_device(np.ascontiguousarray(v.transpose(2, 1, 0))).transpose(2, 1, 0)) for v, _ in small], False)
    # a base one element into its buffer: 2- or 4-byte alignment of every piece load
    off = []
    for v, _ in small:
        buf = to_device(np.concatenate([v.reshape(-1)[:1], v.reshape(-1)]))
        off.append(mark(DeviceArray(buf.ptr + v.itemsize, (w, h, C), v.dtype, 0, owner=buf)))
    fused(off, True)
    # host numpy images, the (h,w,C) view among them
    fused([v for v, _ in small], True)
    fused([np.ascontiguousarray(v.transpose(1, 0, 2)).transpose(1, 0, 2) for v, _ in small], True)


def test_host_images_in_two_staged_chunks_and_weights(sm, oracle):
    C, kind, dtype = 19, "summax", "float16"
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P, n = len(mesh.faces), 11
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], 15)
    rng = np.random.default_rng(5)
    weights = [rng.random((W, H), dtype=np.float32) + np.float32(0.25) for _ in range(n)]
    host = sm.fusion.MeshAggregator(P, C, kind)
    host.fuse_views(r, cams[:n], [v for v, _ in small[:n]], weights, **KW)          # eleven views: two staged chunks
    assert sm._lib.last_fuse_kernel() == SAMPLED
    want = check_against_oracle(oracle, host, P, C, kind, 0.5, oidx[:n], big[:n], 0, weights=weights)
    from semantic_meshes_amd.device import to_device
    dev = sm.fusion.MeshAggregator(P, C, kind)
    dev.fuse_views(r, cams[:n], device(sm, small[:n], dtype), [to_device(x) for x in weights], **KW)
    np.testing.assert_array_equal(bits(dev.get_raw()), bits(want))
    plain = sm.fusion.MeshAggregator(P, C, kind)
    plain.fuse_views(r, cams[:n], device(sm, small[:n], dtype), [to_device(x) for x in weights], resize="bilinear")
    np.testing.assert_array_equal(bits(plain.get_raw()), bits(want))


# ---- 4. special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sum", "summax"])
@pytest.mark.parametrize("dtype", si.DTYPES)
def test_special_values(sm, oracle, dtype, kind):
    """NaN, both infinities, both zeros, binary16 subnormals and all-zero pixels in the source: the bits of the resample-then-fuse
    route, NaNs in the same places."""
    C, n = 19, 4
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.special_images(C, dtype, si.SOURCES["0.37"], n)
    a = sm.fusion.MeshAggregator(P, C, kind)
    a.fuse_views(r, cams[:n], device(sm, small, dtype), **KW)
    assert sm._lib.last_fuse_kernel() == SAMPLED
    b = sm.fusion.MeshAggregator(P, C, kind)
    b.fuse_views(r, cams[:n], device(sm, small, dtype), resize="bilinear")
    got, want = a.get_raw(), b.get_raw()
    nan = np.isnan(want)                          # (a row whose sum is NaN adds nothing: NaN reaches a row only as inf - inf)
    assert (~np.isfinite(want)).any() and not nan.all()
    print("    %d NaN and %d infinite accumulator elements" % (nan.sum(), np.isinf(want).sum()))
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])
    np.testing.assert_array_equal(got, want)      # (equal_nan: assert_array_equal's default)


# ---- 5. the coarse scene: queued triangles, tail waves -----------------------------------------------------------------------------
@pytest.mark.parametrize("iew", si.IEWS)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_coarse_scene(sm, oracle, dtype, iew):
    """helpers.small_scene() as it is: triangles of up to 15 pixels are queued and summed in tree order, so the reference is the
    float64-accumulating oracle, and the two routes through the library agree within the same bound.  The tail waves meet every
    image_equal_weight too."""
    C, kind = 19, "sum"
    mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
    assert sum(queued) > 0
    P, n = len(mesh.faces), len(cams)
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], n)
    a = sm.fusion.MeshAggregator(P, C, kind, iew)
    a.fuse_views(r, cams, device(sm, small, dtype), **KW)
    assert sm._lib.last_fuse_kernel() == SAMPLED
    got = check_against_oracle(oracle, a, P, C, kind, iew, oidx, big, sum(queued))
    b = sm.fusion.MeshAggregator(P, C, kind, iew)
    b.fuse_views(r, cams, device(sm, small, dtype), resize="bilinear")
    assert_fused_close(b.get_raw(), got)


# ---- 6. the other entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_fuse_view_add_many_and_the_render_add_loop(sm, oracle, dtype):
    C, kind, n = 19, "summax", 11
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], 15)
    dev = device(sm, small[:n], dtype)
    ref = sm.fusion.MeshAggregator(P, C, kind)
    ref.fuse_views(r, cams[:n], dev, **KW)
    want = check_against_oracle(oracle, ref, P, C, kind, 0.5, oidx[:n], big[:n], 0)

    one = sm.fusion.MeshAggregator(P, C, kind)
    for k in range(n):
        one.fuse_view(r, cams[k], dev[k], **KW)
        assert not one._pending and sm._lib.last_fuse_kernel() == SAMPLED
    np.testing.assert_array_equal(bits(one.get_raw()), bits(want))

    many = sm.fusion.MeshAggregator(P, C, kind)
    many.add_many([r.render(cam)[0] for cam in cams[:n]], dev, **KW)
    assert sm._lib.last_fuse_kernel() == SAMPLED
    np.testing.assert_array_equal(bits(many.get_raw()), bits(want))

    loop = sm.fusion.MeshAggregator(P, C, kind)

    def run():
        for k in range(n):
            idx, depth = r.render(cams[k])
            loop.add(idx, dev[k], **KW)
            assert not loop._pending
    launches, fused = fuse_slot_counts(sm, run)
    assert (launches, fused) == (n, n)                                      # one launch per view
    assert sm._lib.last_fuse_kernel() == SAMPLED and instance(sm) == (24, 1)
    np.testing.assert_array_equal(bits(loop.get_raw()), bits(want))

    eager = sm.fusion.MeshAggregator(P, C, kind)                            # a plane that was rasterised and looked at: add_sampled
    for k in range(n):
        idx, depth = r.render(cams[k])
        assert np.asarray(idx).shape == (W, H)
        eager.add(idx, dev[k], **KW)
    np.testing.assert_array_equal(bits(eager.get_raw()), bits(want))
    foreign = sm.fusion.MeshAggregator(P, C, kind)                          # an index image from anywhere: resampled, then add()'s path
    for k in range(3):
        foreign.add(oidx[k], small[k][0], **KW, **hh.kw(dtype))
    assert sm._lib.last_fuse_kernel() != SAMPLED
    np.testing.assert_array_equal(bits(foreign.get_raw()), bits(oracle_raw(oracle, P, C, kind, 0.5, oidx[:3], big[:3])[0]))


def test_interleaved_with_deferred_adds_the_order_is_the_callers(sm, oracle):
    """Plain add() calls on lazy planes wait in the aggregator's group; an add() with the keyword hands them over first.
    float32 additions do not commute bit for bit, so the oracle fed the views in the caller's order decides."""
    from semantic_meshes_amd.device import to_device
    C, kind, n = 19, "sum", 9
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, "float32", si.SOURCES["half"], n)
    agg = sm.fusion.MeshAggregator(P, C, kind)
    assert agg.defer
    seen = []
    for k in range(n):
        idx, depth = r.render(cams[k])
        if k % 3 == 2:
            agg.add(idx, marked(sm, small[k][0], "float32"), **KW)
            assert not agg._pending
            seen.append(big[k])
        else:
            full = to_device(big[k])                                        # a camera-resolution image of the library's own: deferred
            agg.add(idx, full)
            assert agg._pending
            seen.append(big[k])
    check_against_oracle(oracle, agg, P, C, kind, 0.5, oidx[:n], seen, 0)


# ---- 7. fallbacks and the hook -----------------------------------------------------------------------------------------------------
def test_mul_falls_back(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    rng = np.random.default_rng(3)
    small = [np.maximum(random_probs(rng, 59, 44, C), np.float32(1e-3)) for _ in range(4)]
    big = [ref.ref_resize(s, W, H) for s in small]
    agg = sm.fusion.MeshAggregator(P, C, "mul")
    agg.fuse_views(r, cams[:4], [marked(sm, s, "float32") for s in small], **KW)
    assert sm._lib.last_fuse_kernel() != SAMPLED
    want = oracle_raw(oracle, P, C, "mul", 0.5, oidx[:4], big, double=True)[1]
    assert_fused_close(agg.get(), want, rtol=1e-5, atol=1e-6)                 # test_fuse_views_resized_mul's bounds


def test_texel_renderer_falls_back(sm, oracle):
    C, n = 19, 3
    mesh, cams, r, oidx, queued = scene(sm, oracle, "small")
    rt = sm.render.texels(mesh, cams, 0.5)
    P = rt.getPrimitivesNum()
    small, big = si.source_images(C, "float16", si.SOURCES["half"], n)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_views(rt, cams[:n], device(sm, small, "float16"), **KW)
    assert sm._lib.last_fuse_kernel() != SAMPLED
    b = sm.fusion.MeshAggregator(P, C)
    b.fuse_views(rt, cams[:n], device(sm, small, "float16"), resize="bilinear")
    assert np.abs(b.get_raw()).sum() > 0
    np.testing.assert_array_equal(bits(a.get_raw()), bits(b.get_raw()))


@pytest.mark.parametrize("dtype", si.DTYPES)
def test_the_hook_sends_every_call_down_the_resampling_route(sm, oracle, dtype):
    C, kind, n = 19, "sum", 11
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, dtype, si.SOURCES["0.37"], 15)
    a = sm.fusion.MeshAggregator(P, C, kind)
    a.fuse_views(r, cams[:n], device(sm, small[:n], dtype), **KW)
    assert sm._lib.last_fuse_kernel() == SAMPLED
    assert sm._lib.get_option("fuse_sampled") == 1
    sm._lib.set_option("fuse_sampled", 0)
    try:
        b = sm.fusion.MeshAggregator(P, C, kind)
        b.fuse_views(r, cams[:n], device(sm, small[:n], dtype), **KW)
        assert sm._lib.last_fuse_kernel() == ("k_fuse_tri" if dtype == "float32" else NATIVE)
        c = sm.fusion.MeshAggregator(P, C, kind)
        for k in range(3):
            idx, depth = r.render(cams[k])
            c.add(idx, marked(sm, small[k][0], dtype), **KW)
        assert sm._lib.last_fuse_kernel() == ("k_fuse_tri" if dtype == "float32" else NATIVE)
    finally:
        sm._lib.set_option("fuse_sampled", 1)
    np.testing.assert_array_equal(bits(b.get_raw()), bits(a.get_raw()))
    np.testing.assert_array_equal(bits(c.get_raw()), bits(oracle_raw(oracle, P, C, kind, 0.5, oidx[:3], big[:3])[0]))


def test_identity_size_passes_through(sm, oracle):
    C, kind, n = 19, "summax", 3
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, "float16", (W, H), n)                    # (ref_resize at equal sizes is the identity)
    for (v, wide), b in zip(small, big):
        np.testing.assert_array_equal(bits(wide), bits(b))
    a = sm.fusion.MeshAggregator(P, C, kind)
    a.fuse_views(r, cams[:n], device(sm, small, "float16"), **KW)
    assert sm._lib.last_fuse_kernel() == NATIVE                               # the existing entry point, the image untouched
    check_against_oracle(oracle, a, P, C, kind, 0.5, oidx[:n], big, 0)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_aggregator_unchanged(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, "float32", si.SOURCES["half"], 8)
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view(r, cams[0], marked(sm, small[0][0], "float32"), **KW)
    before = bits(a.get_raw()).copy()
    assert before.any()
    good, wrong = marked(sm, small[1][0], "float32"), marked(sm, np.ascontiguousarray(small[1][0][:, :, :-1]), "float32")
    for bad, kwargs in ((wrong, {"resize": "bilinear"}), (good, {"resize": "nearest"}), (good, {}),
                        (marked(sm, small[1][0].astype(np.float64), "float32"), {"resize": "bilinear"})):
        kwargs = dict(kwargs, sample_in_kernel=True)      # ((good, {}) is the keyword without resize=)
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


def test_the_c_entry_points_refuse_bad_arguments(sm, oracle):
    L, lib = sm._lib, sm._lib.lib()
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    P = len(mesh.faces)
    small, big = si.source_images(C, "float32", si.SOURCES["half"], 8)
    w, h = si.SOURCES["half"]
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view(r, cams[0], marked(sm, small[0][0], "float32"), **KW)
    before = bits(a.get_raw()).copy()
    src = marked(sm, small[1][0], "float32")
    pod = cams[1]._pod
    pp = (ctypes.c_void_p * 1)(src.ptr)
    idx = r.render(cams[1])[0]
    for dt, mode, ww, hh_ in ((7, L.RESIZE_BILINEAR, w, h), (L.PROBS_F32, 0, w, h), (L.PROBS_F32, L.RESIZE_BILINEAR, 0, h),
                              (L.PROBS_F32, L.RESIZE_BILINEAR, w, 0), (L.PROBS_F32, L.RESIZE_BILINEAR, 65537, h)):
        for call in (lambda: lib.smesh_fuse_views_sampled(r._h, a._h, ctypes.byref(pod), 1, pp, dt, None, ww, hh_, None, L.MEM_DEVICE, mode),
                     lambda: lib.smesh_fuse_view_sampled(r._h, a._h, ctypes.byref(pod), ctypes.c_void_p(src.ptr), dt, None, ww, hh_, None, L.MEM_DEVICE, mode),
                     lambda: lib.smesh_aggregator_add_sampled(a._h, r._h, ctypes.c_void_p(idx.ptr), L.IDX_U32, None, L.MEM_DEVICE,
                                                              ctypes.c_void_p(src.ptr), dt, None, L.MEM_DEVICE, None, None, L.MEM_HOST,
                                                              ww, hh_, W, H, mode)):
            assert call() == L.ERR_INVALID and lib.smesh_last_error()
    # the class count is the aggregator's: one with C == 0 cannot be made
    h0 = ctypes.c_void_p()
    assert lib.smesh_aggregator_create(P, 0, L.AGG_KINDS["Sum"], 0.5, 0, ctypes.byref(h0)) == L.ERR_INVALID and lib.smesh_last_error()
    assert lib.smesh_fuse_views_sampled(r._h, a._h, ctypes.byref(pod), 1, pp, L.PROBS_F16, None, w, h, None, L.MEM_DEVICE + 7, L.RESIZE_BILINEAR) == L.ERR_INVALID
    odd = ctypes.c_void_p(src.ptr + 2)                                        # a float32 image at a 2-byte address
    assert lib.smesh_fuse_view_sampled(r._h, a._h, ctypes.byref(pod), odd, L.PROBS_F32, None, w, h, None, L.MEM_DEVICE, L.RESIZE_BILINEAR) == L.ERR_INVALID
    np.testing.assert_array_equal(bits(a.get_raw()), before)
