"""Images from cameras with lens distortion, undistorted on the GPU (include/smesh_lens.h): every entry point against lens_ref.py --
the numpy restatement of DESIGN.md 3.18, which tests/test_lens_host.py checks on its own -- bit for bit.  Fusion is the CPU oracle
fed the restatement's images and weights, and the library fed the planes of `undistort_probs_device` by hand."""
import ctypes

import numpy as np
import pytest

import half_helpers as hh
import lens_ref as lr
import resize_ref as rref
from helpers import assert_fused_close, random_probs
from test_gpu_half import check_against_oracle, oracle_raw, scene
from test_gpu_labels import bits
from test_gpu_resize import layouts

pytestmark = pytest.mark.gpu

# source (w,h) -> view (W,H); the calibration size is the view's
BELOW_A_WAVE = ((30, 8), (90, 20))          # H = 20: a wave of the pixel kernel spans more than three columns
BEYOND_A_RUN = ((45, 39), (140, 300))       # H = 300 > 256, the longest run of pixels a workgroup of k_undistort_probs maps
SHAPES = (((64, 48), (64, 48)), ((32, 24), (64, 48)), ((40, 27), (67, 45)), ((37, 53), (130, 67)), BELOW_A_WAVE, BEYOND_A_RUN)
SMALL_SHAPES = SHAPES[:4]
# The launch code's other thresholds, by class count on these shapes (float32): 4 classes on H = 48 are 48 pieces a column -- one
# workgroup a column, and fewer pieces than lanes; 40 classes are ten pieces a pixel, 480 a column -- two workgroups, and 256 is no
# multiple of ten, so a pixel's pieces straddle them; 67 columns of one or three workgroups are no multiple of the eight XCDs the
# grid is rounded to; 3015 pixels are no multiple of the pixel kernel's 256.  1, 3, 5, 19 and 41 classes are no multiple of a lane's
# four (float32) or eight (16 bit) elements: the generic path whatever "lens_vector" says.
CLASSES = (1, 3, 4, 5, 8, 19, 40, 41)
_cache = {}


def shape_id(shape):
    return "%dx%d-%dx%d" % (shape[0] + shape[1])


@pytest.fixture(params=[1, 0], ids=["vector", "generic"])
def vector(sm, request):
    before = sm._lib.get_option("lens_vector")
    sm._lib.set_option("lens_vector", request.param)
    yield request.param
    sm._lib.set_option("lens_vector", before)


def cam_of(sm, lens, view=None, pose=None):
    """The data.LensCamera of a restated lens (and view; None: the default one)."""
    R, t = (np.eye(3), np.zeros(3)) if pose is None else pose
    model = lens["model"]
    params = lr.distortion_params(model, [lens["k"][i] for i in lr.SLOTS[model][0]], [lens["p"][i] for i in lr.SLOTS[model][1]])
    kw = {} if view is None else dict(view_focal_lengths=view["F"], view_principal_point=view["P"], view_resolution=np.array(view["size"]))
    return sm.data.LensCamera(R, t, np.array(lens["size"]), lens["f"], lens["c"], model, params, **kw)


def source(w, h, C, dtype, special=False):
    key = ("src", w, h, C, dtype, special)
    if key not in _cache:
        rng = np.random.default_rng(w * 100003 + h * 1009 + C * 7 + rref.DTYPES.index(dtype) + 12345)
        if special:      # NaN, both infinities and -0.0 in the middle of the image, where every lens samples
            p = rref.make_source(rng, w, h, C, "float32")[0].copy()
            for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
                p[w // 2 + k - 2, h // 2 + (k % 2), k % C] = v
            b = None if dtype == "float32" else hh.narrow(p, dtype)
            _cache[key] = (p, p) if b is None else (hh.typed(b, dtype), hh.widen(b, dtype))
        else:
            _cache[key] = rref.make_source(rng, w, h, C, dtype)
    return _cache[key]


def undistorted(w, h, C, dtype, index, W, H, special=False):
    """(float32 image, inside) of the restatement for that source, test lens `index` and its default view, computed once."""
    key = ("ref", w, h, C, dtype, index, W, H, special)
    if key not in _cache:
        lens = lr.test_lens(index, W, H)
        _cache[key] = lr.ref_undistort_probs(source(w, h, C, dtype, special)[1], lens, lr.default_view(lens))
    return _cache[key]


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def got_bits(out, out_dtype):
    a = np.asarray(out)
    return f32_bits(a) if out_dtype == "float32" else a.view(np.uint16)


def want_bits(wide, out_dtype):
    return f32_bits(wide) if out_dtype == "float32" else hh.narrow(wide, out_dtype)


def check_probs(sm, image, cam, want, inside, dtype="float32", out_dtype=None, weights_image=None, **kw):
    out, wts, counts = sm.fusion.undistort_probs_device(image, cam, out_dtype=out_dtype, weights_image=weights_image, return_weights=True,
                                                         return_counts=True, **kw)
    W, H = cam.resolution
    od = out_dtype or dtype
    assert type(out).__name__ == "DeviceArray" and out.shape == want.shape and out.strides == (H * want.shape[2], want.shape[2], 1)
    assert out.dtype == {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[od] and out.bfloat16 == (od == "bfloat16")
    assert np.array_equal(got_bits(out, od), want_bits(want, od))
    assert wts.shape == (W, H) and wts.dtype == np.float32
    assert np.array_equal(f32_bits(wts), f32_bits(lr.ref_weights(inside, weights_image)))
    assert counts.tolist() == lr.ref_counts(inside).tolist()


# ---- 1. smesh_undistort_probs / undistort_probs_device -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_float32_at_every_shape_lens_and_class_count(sm, vector, shape):
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = shape
    outside = []
    for index in range(len(lr.TEST_LENSES)):
        cam = cam_of(sm, lr.test_lens(index, W, H))
        for C in (CLASSES if index in (1, 4) else (5, 8)):
            if shape == BEYOND_A_RUN and C not in (4, 5, 8, 40):
                continue
            want, inside = undistorted(w, h, C, "float32", index, W, H)
            check_probs(sm, to_device(source(w, h, C, "float32")[0]), cam, want, inside)
        outside.append(int((~inside).sum()))
        assert 2 * outside[-1] <= W * H                 # the inside branch: no lens leaves fewer than half its pixels inside
    assert max(outside) > 0                             # the outside branch: some lens has outside pixels on every shape
    if shape in SMALL_SHAPES:
        assert outside == [0, {3072: 313, 3015: 303, 8710: 738}[W * H], 0, 0, 0]


@pytest.mark.parametrize("out_dtype", rref.DTYPES)
@pytest.mark.parametrize("in_dtype", rref.DTYPES)
def test_all_nine_dtype_pairs(sm, vector, in_dtype, out_dtype):
    from semantic_meshes_amd.device import to_device
    for (w, h), (W, H) in SMALL_SHAPES[1:]:
        for index in (1, 3):
            cam = cam_of(sm, lr.test_lens(index, W, H))
            for C in (8, 19):
                want, inside = undistorted(w, h, C, in_dtype, index, W, H)
                check_probs(sm, to_device(source(w, h, C, in_dtype)[0]), cam, want, inside, in_dtype, out_dtype, **hh.kw(in_dtype))
                if in_dtype == out_dtype:      # the default out_dtype is the input's; the bare image is what comes back
                    same = sm.fusion.undistort_probs(to_device(source(w, h, C, in_dtype)[0]), cam, **hh.kw(in_dtype))
                    assert np.array_equal(got_bits(same, out_dtype), want_bits(want, out_dtype))


@pytest.mark.parametrize("dtype", rref.DTYPES)
def test_layouts_and_host_images(sm, vector, dtype):
    for (w, h), (W, H) in (SMALL_SHAPES[1], SMALL_SHAPES[2]):
        cam = cam_of(sm, lr.test_lens(1, W, H))
        for C in (8, 19):
            values, wide = source(w, h, C, dtype)
            want, inside = undistorted(w, h, C, dtype, 1, W, H)
            for name, dev, host in layouts(sm, values, dtype):
                check_probs(sm, dev, cam, want, inside, dtype, **hh.kw(dtype))
                if host is not None:          # a host image gives what the device image gives
                    check_probs(sm, host, cam, want, inside, dtype, **hh.kw(dtype))


@pytest.mark.parametrize("dtype", rref.DTYPES)
def test_nan_and_infinities_in_the_source(sm, vector, dtype):
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = SMALL_SHAPES[2]
    for index in (1, 4):
        cam = cam_of(sm, lr.test_lens(index, W, H))
        for C in (5, 8):
            want, inside = undistorted(w, h, C, dtype, index, W, H, special=True)
            assert np.isnan(want).any() and np.isinf(want).any()
            check_probs(sm, to_device(source(w, h, C, dtype, special=True)[0]), cam, want, inside, dtype, **hh.kw(dtype))


def test_weights_images_and_another_view(sm, vector):
    """The caller's (W,H) weights are multiplied in, from host and device; a view camera that is not the default -- F = 0.9 f, a
    shifted P, another size than the calibration's -- maps through its own F and P."""
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(3)
    (w, h), (W, H) = SMALL_SHAPES[2]
    for index in (1, 3, 4):
        lens = lr.test_lens(index, W, H)
        for view in (None, lr.make_view(0.9 * lens["f"], lens["c"] + np.array([2.5, -1.5]), (W + 6, H - 4))):
            cam = cam_of(sm, lens, view)
            VW, VH = cam.resolution
            w_in = rng.uniform(0.0, 2.0, size=(VW, VH)).astype(np.float32)
            for C in (8, 19):
                values, wide = source(w, h, C, "float32")
                want, inside = lr.ref_undistort_probs(wide, lens, view or lr.default_view(lens))
                assert 0 < (~inside).sum() or index != 1
                check_probs(sm, to_device(values), cam, want, inside, weights_image=w_in)
                check_probs(sm, values, cam, want, inside, weights_image=to_device(w_in))
                check_probs(sm, values, cam, want, inside)


def test_the_path_a_launch_takes(sm):
    """With "lens_vector" on, 8 and 40 classes (and 8 in 16 bits) run the vector form of k_undistort_probs, 19 classes, a channel-first
    tensor and an image one element into its buffer the generic form; with it off everything does.  The nearest kernel reports itself."""
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = SMALL_SHAPES[2]
    cam = cam_of(sm, lr.test_lens(1, W, H))
    before = sm._lib.get_option("lens_vector")
    try:
        for on in (1, 0):
            sm._lib.set_option("lens_vector", on)
            for C, dtype, want in ((8, "float32", 1), (40, "float32", 1), (8, "float16", 1), (19, "float32", 2), (4, "float16", 2)):
                sm.fusion.undistort_probs_device(to_device(source(w, h, C, dtype)[0]), cam)
                assert sm._lib.get_option("last_lens_path") == (want if on else 2), (on, C, dtype)
            values = source(w, h, 8, "float32")[0]
            for name, dev, host in layouts(sm, values, "float32"):
                sm.fusion.undistort_probs_device(dev, cam)
                assert sm._lib.get_option("last_lens_path") == (1 if on and name in ("dense", "hwc") else 2), (on, name)
        sm.fusion.undistort_labels_device(np.zeros((w, h), np.uint8), cam, 255)
        assert sm._lib.get_option("last_lens_path") == 3
    finally:
        sm._lib.set_option("lens_vector", before)


def lens_pod(sm, lens):
    return cam_of(sm, lens).lens._pod


def test_the_c_entry_points_refuse_and_touch_nothing(sm):
    from semantic_meshes_amd.device import to_device
    L = sm._lib.lib()
    w, h, C, W, H = 8, 6, 4, 16, 12
    lens = lr.test_lens(3, W, H)
    cam = cam_of(sm, lens)
    src = to_device(np.ones((w, h, C), np.float32))
    out = to_device(np.full((W, H, C), 7, np.float32))
    mask, mout = to_device(np.ones((w, h), np.uint8)), to_device(np.full((W, H), 9, np.uint8))
    fill = np.zeros(4, np.uint8)
    c64 = lambda v: (ctypes.c_int64 * 3)(*v)
    p = lambda a: ctypes.c_void_p(a.ptr)

    def probs(in_=src, idt=0, strides=None, mem=1, w_=w, h_=h, C_=C, lens_=None, view=None, out_=out, odt=0):
        lp = cam.lens._pod if lens_ is None else lens_
        vp = cam._pod if view is None else view
        return L.smesh_undistort_probs(None if in_ is None else p(in_), idt, strides, mem, w_, h_, C_, ctypes.byref(lp) if lp else None,
                                       ctypes.byref(vp) if vp else None, None if out_ is None else p(out_), odt, None, None, None, 0)

    def pixels(in_=mask, eb=1, ch=1, strides=None, mem=1, w_=w, h_=h, lens_=None, out_=mout, fill_=fill):
        lp = cam.lens._pod if lens_ is None else lens_
        return L.smesh_undistort_pixels(None if in_ is None else p(in_), eb, ch, strides, mem, w_, h_, ctypes.byref(lp), ctypes.byref(cam._pod),
                                        None if fill_ is None else fill_.ctypes.data_as(ctypes.c_void_p), None if out_ is None else p(out_), None, 0)

    def bad_lens(**kw):
        pod = sm._lib.LensPOD.from_buffer_copy(cam.lens._pod)
        for name, (i, v) in kw.items():
            getattr(pod, name)[i] = v
        return pod

    big = sm._lib.CameraPOD.from_buffer_copy(cam._pod)
    big.width = 65537
    nofocal = sm._lib.CameraPOD.from_buffer_copy(cam._pod)
    nofocal.focal[1] = 0.0
    refused = [probs(in_=None), probs(out_=None), probs(idt=3), probs(odt=-1), probs(strides=c64((-1, 1, 1))), probs(mem=2), probs(w_=0),
               probs(h_=0), probs(C_=0), probs(w_=65537), probs(view=big), probs(view=nofocal), probs(lens_=bad_lens(k=(2, float("nan")))),
               probs(lens_=bad_lens(p=(1, float("inf")))), probs(lens_=bad_lens(focal=(0, 0.0))), probs(lens_=bad_lens(focal=(1, -1.0))),
               probs(lens_=bad_lens(principal=(0, float("nan")))), probs(out_=src, w_=4, h_=3),
               pixels(in_=None), pixels(out_=None), pixels(fill_=None), pixels(eb=3), pixels(ch=0), pixels(ch=5), pixels(strides=c64((1, -1, 0))),
               pixels(w_=0), pixels(lens_=bad_lens(k=(0, float("inf")))), pixels(out_=mask, w_=4, h_=3)]
    assert all(s == sm._lib.ERR_INVALID for s in refused), refused
    kept = np.array([5, 6], np.uint64)                              # a refused call leaves the caller's counts alone too
    assert L.smesh_undistort_probs(p(src), 0, None, 1, w, h, C, ctypes.byref(cam.lens._pod), ctypes.byref(cam._pod), None, 0, None, None,
                                   kept.ctypes.data_as(ctypes.c_void_p), 0) == sm._lib.ERR_INVALID
    assert L.smesh_undistort_pixels(p(mask), 1, 1, None, 1, w, h, ctypes.byref(cam.lens._pod), ctypes.byref(cam._pod),
                                    fill.ctypes.data_as(ctypes.c_void_p), None, kept.ctypes.data_as(ctypes.c_void_p), 0) == sm._lib.ERR_INVALID
    assert kept.tolist() == [5, 6]
    assert sm._lib.lib().smesh_last_error()
    assert (np.asarray(out) == 7).all() and (np.asarray(mout) == 9).all() and (np.asarray(src) == 1).all()
    before = sm._lib.get_option("lens_launches")
    assert probs() == 0 and pixels() == 0
    assert sm._lib.get_option("lens_launches") == before + 2
    with pytest.raises(ValueError):
        sm._lib.set_option("lens_launches", 0)
    with pytest.raises(ValueError):
        sm.fusion.undistort_probs_device(src, sm.data.Camera(np.eye(3), np.zeros(3), np.array([W, H]), lens["f"], lens["c"]))


# ---- 2. smesh_undistort_pixels / undistort_labels_device / undistort_depth_device ----------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_masks_of_every_dtype(sm, shape):
    from semantic_meshes_amd.device import to_device
    (w, h), (W, H) = shape
    rng = np.random.default_rng(w + h)
    for index in range(len(lr.TEST_LENSES)):
        lens = lr.test_lens(index, W, H)
        cam = cam_of(sm, lens)
        for dt, fill in ((np.uint8, 255), (np.int16, -1), (np.uint16, 65535), (np.int32, -7), (np.int64, -(2 ** 40))):
            info = np.iinfo(dt)
            mask = rng.integers(max(info.min, -2 ** 62), min(info.max, 2 ** 62), size=(w, h), dtype=np.int64).astype(dt)
            want, inside = lr.ref_undistort_pixels(mask, lens, lr.default_view(lens), fill)
            for image in (mask, to_device(mask)):
                out, counts = sm.fusion.undistort_labels_device(image, cam, fill, return_counts=True)
                assert out.shape == (W, H) and out.dtype == np.dtype(dt) and out.strides == (H, 1)
                assert np.array_equal(np.asarray(out), want)
                assert counts.tolist() == lr.ref_counts(inside).tolist()
            decoded = np.ascontiguousarray(mask.T)                   # a decoded (h,w) image as its transposed view
            assert np.array_equal(sm.fusion.undistort_labels(decoded.T, cam, fill), want)
            assert np.array_equal(sm.fusion.undistort_labels(to_device(decoded).transpose(1, 0), cam, fill), want)


def test_colour_masks_and_sensor_depth(sm):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(11)
    for (w, h), (W, H) in (SMALL_SHAPES[1], SMALL_SHAPES[2]):
        for index in (1, 4):
            lens = lr.test_lens(index, W, H)
            cam, view = cam_of(sm, lens), lr.default_view(lens)
            for ch in (3, 4):
                decoded = rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8)     # (h,w,ch) as an image decoder leaves it
                fill = np.arange(250, 250 + ch).astype(np.uint8)
                want, inside = lr.ref_undistort_pixels(decoded.transpose(1, 0, 2), lens, view, fill)
                for image in (decoded.transpose(1, 0, 2), to_device(decoded).transpose(1, 0, 2), np.ascontiguousarray(decoded.transpose(1, 0, 2))):
                    out = sm.fusion.undistort_labels_device(image, cam, fill)
                    assert out.shape == (W, H, ch) and out.strides == (H * ch, ch, 1)
                    assert np.array_equal(np.asarray(out), want)
                one = sm.fusion.undistort_labels(decoded.transpose(1, 0, 2), cam, 255)           # one value for every channel
                assert np.array_equal(one, lr.ref_undistort_pixels(decoded.transpose(1, 0, 2), lens, view, np.full(ch, 255, np.uint8))[0])
            for depth in (rng.integers(1, 65536, size=(w, h)).astype(np.uint16), rng.uniform(0.1, 9.0, size=(w, h)).astype(np.float32)):
                want, inside = lr.ref_undistort_pixels(depth, lens, view, 0)
                for image in (depth, to_device(depth)):
                    out = sm.fusion.undistort_depth_device(image, cam)
                    assert out.dtype == depth.dtype and np.array_equal(np.asarray(out).view(np.uint8), want.view(np.uint8))
                assert index != 1 or (np.asarray(out)[~inside] == 0).all()
            with pytest.raises(ValueError):
                sm.fusion.undistort_depth_device(depth.astype(np.float64), cam)
            with pytest.raises(ValueError):
                sm.fusion.undistort_labels_device(np.zeros((w, h), np.uint8), cam, 256)


@pytest.mark.parametrize("index", range(len(lr.TEST_LENSES)))
def test_the_direction_on_the_device(sm, index):
    """A 3 x 3 blob of its own label painted where COLMAP's forward projection puts each of a dozen 3-D points, on an otherwise
    don't-care mask: after undistort_labels_device the pinhole pixel of each point carries the point's label."""
    model, k, p = lr.TEST_LENSES[index]
    W, H = 130, 67
    lens = lr.test_lens(index, W, H)
    cam = cam_of(sm, lens)
    F, P = cam.focal_lengths, cam.principal_point
    mask = np.full((W, H), 255, np.uint8)
    points = []
    for j, (gx, gy) in enumerate([(a, b) for a in (-0.42, -0.15, 0.12, 0.4) for b in (-0.2, 0.02, 0.21)]):      # a dozen, inside the image
        Z = 1.5 + 0.25 * j
        point = (gx * Z, gy * Z, Z)
        u, v = lr.colmap_project(model, lens["f"], lens["c"], lr.distortion_params(model, k, p), point)
        iu, iv = int(np.floor(u)), int(np.floor(v))
        assert 1 <= iu < W - 1 and 1 <= iv < H - 1
        assert (mask[iu - 1:iu + 2, iv - 1:iv + 2] == 255).all()     # the blobs do not touch
        mask[iu - 1:iu + 2, iv - 1:iv + 2] = j
        points.append((j, int(np.floor(F[0] * gx + P[0])), int(np.floor(F[1] * gy + P[1]))))
    out = sm.fusion.undistort_labels(mask, cam, 255)
    for j, X, Y in points:
        assert 0 <= X < W and 0 <= Y < H and out[X, Y] == j, (model, j, X, Y, out[X, Y])


# ---- 3. fusion -------------------------------------------------------------------------------------------------------------------
VIEWS = 11                                   # one chunk of eight and a tail
W, H = 160, 120
SOURCES = {"full": (160, 120), "0.6": (96, 72)}


def lens_scene(sm, oracle):
    """test_gpu_half.scene("fine") with its first eleven cameras made into LensCameras: the camera's own f and c, the test lenses'
    distortion in turn -- (cameras, restated lenses, restated views)."""
    if "scene" not in _cache:
        mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
        lcams, lenses, views = [], [], []
        for i, cam in enumerate(cams[:VIEWS]):
            model, k, p = lr.TEST_LENSES[(i + 1) % len(lr.TEST_LENSES)]
            lens = lr.make_lens(model, cam.focal_lengths, cam.principal_point, k, p, (W, H))
            lc = cam_of(sm, lens, pose=(cam.rotation, cam.translation))
            assert bytes(lc._pod) == bytes(cam._pod)        # the default view is the scene's pinhole camera: the same render
            lcams.append(lc)
            lenses.append(lens)
            views.append(lr.default_view(lens))
        _cache["scene"] = (lcams, lenses, views)
    return _cache["scene"]


def fusion_images(sm, oracle, C, dtype, size, positive=False):
    """Per view: (values, widened) of a source image at `size`, what the fusion must see -- the restatement's image rounded to the
    input's dtype and widened again -- and the restatement's weights."""
    key = ("fimg", C, dtype, size, positive)
    if key not in _cache:
        lcams, lenses, views = lens_scene(sm, oracle)
        w, h = size
        rng = np.random.default_rng(1000 * C + 13 * w + rref.DTYPES.index(dtype))
        small, big, wts = [], [], []
        for lens, view in zip(lenses, views):
            if dtype == "float32":
                values = wide = np.maximum(random_probs(rng, w, h, C), np.float32(1e-3)) if positive else random_probs(rng, w, h, C)
            else:
                b = hh.random_probs16(rng, w, h, C, dtype)
                values, wide = hh.typed(b, dtype), hh.widen(b, dtype)
            small.append((values, wide))
            out, inside = lr.ref_undistort_probs(wide, lens, view)
            big.append(out if dtype == "float32" else hh.widen(hh.narrow(out, dtype), dtype))
            wts.append(lr.ref_weights(inside))
        assert any((x == 0).any() for x in wts) and all(2 * int((x == 0).sum()) < x.size for x in wts)
        _cache[key] = (small, big, wts)
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
def test_fuse_views_undistorted_against_the_oracle_and_the_planes_by_hand(sm, oracle, dtype, kind, C, size):
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")      # no queued triangles: one lane owns a row, the oracle's bits
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    small, big, wts = fusion_images(sm, oracle, C, dtype, SOURCES[size])
    iew = [0.0, 0.5, 1.0][(C + len(kind)) % 3]
    a = sm.fusion.MeshAggregator(P, C, kind, iew)
    a.fuse_views(r, lcams, [marked(sm, v, dtype) for v, _ in small], undistort=True, **hh.kw(dtype))
    got = check_against_oracle(oracle, a, P, C, kind, iew, oidx[:VIEWS], big, 0, weights=wts)
    b = sm.fusion.MeshAggregator(P, C, kind, iew)
    pre = [sm.fusion.undistort_probs_device(marked(sm, v, dtype), cam, return_weights=True, **hh.kw(dtype)) for (v, _), cam in zip(small, lcams)]
    assert all(p.dtype == small[0][0].dtype and p.shape == (W, H, C) and q.shape == (W, H) for p, q in pre)
    b.fuse_views(r, lcams, [p for p, _ in pre], [q for _, q in pre], **hh.kw(dtype))
    np.testing.assert_array_equal(bits(b.get_raw()), bits(got))
    if dtype == "float32" and kind == "sum":                     # host images, view by view, and with the caller's weights
        c = sm.fusion.MeshAggregator(P, C, kind, iew)
        for k in range(VIEWS):
            c.fuse_view(r, lcams[k], small[k][0], undistort=True)
        np.testing.assert_array_equal(bits(c.get_raw()), bits(got))
        rng = np.random.default_rng(8)
        mine = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) for _ in range(VIEWS)]
        d = sm.fusion.MeshAggregator(P, C, kind, iew)
        d.fuse_views(r, lcams, [v for v, _ in small], mine, undistort=True)
        check_against_oracle(oracle, d, P, C, kind, iew, oidx[:VIEWS], big, 0, weights=[x * y for x, y in zip(mine, wts)])


@pytest.mark.parametrize("C", [19, 40])
def test_fuse_views_undistorted_mul(sm, oracle, C):
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    small, big, wts = fusion_images(sm, oracle, C, "float32", SOURCES["0.6"], positive=True)
    agg = sm.fusion.MeshAggregator(P, C, "mul")
    agg.fuse_views(r, lcams, [marked(sm, v, "float32") for v, _ in small], undistort=True)
    want = oracle_raw(oracle, P, C, "mul", 0.5, oidx[:VIEWS], big, weights=wts, double=True)[1]
    assert_fused_close(agg.get(), want, rtol=1e-5, atol=1e-6)
    by_hand = sm.fusion.MeshAggregator(P, C, "mul")
    pre = [sm.fusion.undistort_probs_device(v, cam, return_weights=True) for (v, _), cam in zip(small, lcams)]
    by_hand.fuse_views(r, lcams, [p for p, _ in pre], [q for _, q in pre])
    np.testing.assert_array_equal(bits(by_hand.get_raw()), bits(agg.get_raw()))


def test_fuse_views_labels_undistorted_with_a_map_and_a_palette(sm, oracle):
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    rng = np.random.default_rng(21)
    w, h = SOURCES["0.6"]
    table = rng.integers(-1, C, size=256).astype(np.int32)           # a full table: every uint8 value is inside it
    masks = [rng.integers(0, 256, size=(w, h)).astype(np.uint8) for _ in range(VIEWS)]
    classes = [np.where((table[m] >= 0), table[m], 255).astype(np.uint8) for m in masks]      # mapped at the mask's own size
    planes = [lr.ref_undistort_pixels(c, lens, view, 255)[0] for c, lens, view in zip(classes, lenses, views)]
    assert any((lr.lens_map(lens, view, w, h)[2] == 0).any() for lens, view in zip(lenses, views))
    want = sm.fusion.MeshAggregator(P, C)
    want.fuse_views_labels(r, lcams, planes)
    assert np.abs(want.get_raw()).sum() > 0
    for images in (masks, [to_device(m) for m in masks]):
        a = sm.fusion.MeshAggregator(P, C)
        a.fuse_views_labels(r, lcams, images, undistort=True, label_map=table)
        np.testing.assert_array_equal(bits(a.get_raw()), bits(want.get_raw()))
    # without a map: the raw values are the classes, everything else (the fill included) is don't care
    raw = sm.fusion.MeshAggregator(P, C)
    raw.fuse_views_labels(r, lcams, [c.astype(np.int32) for c in classes], undistort=True)
    np.testing.assert_array_equal(bits(raw.get_raw()), bits(want.get_raw()))
    one = sm.fusion.MeshAggregator(P, C)
    for k in range(VIEWS):
        one.fuse_view_labels(r, lcams[k], masks[k], undistort=True, label_map=table)
    np.testing.assert_array_equal(bits(one.get_raw()), bits(want.get_raw()))
    # colour masks: class = row of the palette, a colour outside it is don't care
    palette = rng.integers(0, 256, size=(C, 3)).astype(np.uint8)
    assert len({tuple(c) for c in palette}) == C and (1, 1, 1) not in {tuple(c) for c in palette}
    ids = [rng.integers(0, C + 3, size=(w, h)) for _ in range(VIEWS)]
    colours = [np.where((i < C)[:, :, None], palette[np.minimum(i, C - 1)], np.uint8(1)).astype(np.uint8) for i in ids]
    cplanes = [lr.ref_undistort_pixels(np.where(i < C, i, 255).astype(np.uint8), lens, view, 255)[0] for i, lens, view in zip(ids, lenses, views)]
    cwant = sm.fusion.MeshAggregator(P, C)
    cwant.fuse_views_labels(r, lcams, cplanes)
    decoded = [np.ascontiguousarray(c.transpose(1, 0, 2)) for c in colours]               # (h,w,3), handed over as transposed views
    got = sm.fusion.MeshAggregator(P, C)
    got.fuse_views_labels(r, lcams, [d.transpose(1, 0, 2) for d in decoded], undistort=True, palette=palette)
    np.testing.assert_array_equal(bits(got.get_raw()), bits(cwant.get_raw()))


def test_label_views_undistorted_with_host_and_device_weights(sm, oracle):
    """`weights_images` stay (W,H) planes of the view, in host or device memory whatever memory the masks are in: the sums are those of
    the planes fused by hand with the same weights, in bits."""
    from semantic_meshes_amd.device import to_device
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    rng = np.random.default_rng(41)
    w, h = SOURCES["0.6"]
    masks = [rng.integers(0, C + 2, size=(w, h)).astype(np.uint8) for _ in range(VIEWS)]
    weights = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) for _ in range(VIEWS)]
    planes = [lr.ref_undistort_pixels(m, lens, view, 255)[0] for m, lens, view in zip(masks, lenses, views)]
    want = sm.fusion.MeshAggregator(P, C)
    want.fuse_views_labels(r, lcams, planes, weights)
    plain = sm.fusion.MeshAggregator(P, C)
    plain.fuse_views_labels(r, lcams, planes)
    assert not np.array_equal(bits(want.get_raw()), bits(plain.get_raw()))       # the weights count
    table = np.arange(C + 2).astype(np.int32)
    table[C:] = -1
    for images in (masks, [to_device(m) for m in masks]):
        for wts in (weights, [to_device(x) for x in weights]):
            for kwargs in ({}, {"label_map": table}):
                a = sm.fusion.MeshAggregator(P, C)
                a.fuse_views_labels(r, lcams, images, wts, undistort=True, **kwargs)
                np.testing.assert_array_equal(bits(a.get_raw()), bits(want.get_raw()))
            one = sm.fusion.MeshAggregator(P, C)
            for k in range(VIEWS):
                one.fuse_view_labels(r, lcams[k], images[k], wts[k], undistort=True)
            np.testing.assert_array_equal(bits(one.get_raw()), bits(want.get_raw()))
    # a bad image in the second chunk is refused before the first chunk is fused
    bad = sm.fusion.MeshAggregator(P, C)
    with pytest.raises(ValueError):
        bad.fuse_views_labels(r, lcams, masks[:9] + [masks[9].astype(np.float32)] + masks[10:], undistort=True)
    assert not np.abs(bad.get_raw()).sum()


def test_sensor_depths_undistorted_with_a_depth_gate(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    small, big, wts = fusion_images(sm, oracle, C, "float32", SOURCES["0.6"])
    gate = sm.fusion.DepthGate(abs_tol=0.05, rel_tol=0.02)
    # the rendered depth of each view stands for a sensor image on the sensor's grid: undistorted it agrees in the middle only
    sensors = [np.nan_to_num(np.asarray(r.render(cam)[1]), nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32) for cam in lcams]
    a = sm.fusion.MeshAggregator(P, C)
    stats = a.fuse_views(r, lcams, [v for v, _ in small], undistort=True, sensor_depths=sensors, depth_gate=gate, depth_stats=True)
    b = sm.fusion.MeshAggregator(P, C)
    pre = [sm.fusion.undistort_probs_device(v, cam, return_weights=True) for (v, _), cam in zip(small, lcams)]
    depth = [sm.fusion.undistort_depth_device(s, cam) for s, cam in zip(sensors, lcams)]
    for d, s, lens, view in zip(depth, sensors, lenses, views):
        assert np.array_equal(np.asarray(d), lr.ref_undistort_pixels(s, lens, view, 0)[0])
    want = b.fuse_views(r, lcams, [p for p, _ in pre], [q for _, q in pre], sensor_depths=depth, depth_gate=gate, depth_stats=True)
    assert stats.shape == (VIEWS, 4) and np.array_equal(stats, want)
    assert stats[:, 0].min() > 0 and stats[:, 1:].sum() > 0                # every view sees the mesh; the gate closes somewhere
    np.testing.assert_array_equal(bits(a.get_raw()), bits(b.get_raw()))
    one = sm.fusion.MeshAggregator(P, C)
    single = one.fuse_view(r, lcams[0], small[0][0], undistort=True, sensor_depth=sensors[0], depth_gate=gate, depth_stats=True)
    assert single.shape == (4,) and np.array_equal(single, stats[0])


def test_ground_truth_undistorted(sm, oracle):
    from semantic_meshes_amd.fusion import ConfusionMatrix
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    rng = np.random.default_rng(31)
    w, h = SOURCES["0.6"]
    labels = rng.integers(-1, C, size=P).astype(np.int32)
    table = rng.integers(-1, C, size=256).astype(np.int32)
    gts = [rng.integers(0, 256, size=(w, h)).astype(np.uint8) for _ in range(VIEWS)]
    mapped = [np.where(table[g] >= 0, table[g], 255).astype(np.uint8) for g in gts]
    planes = [lr.ref_undistort_pixels(m, lens, view, 255)[0] for m, lens, view in zip(mapped, lenses, views)]
    want = ConfusionMatrix(C)
    want.add_views(r, lcams, labels, planes)
    assert want.get().sum() > 0 and want.ignored > 0
    got = ConfusionMatrix(C)
    got.add_views(r, lcams, labels, gts, gt_map=table, gt_undistort=True)
    np.testing.assert_array_equal(got.get(), want.get())
    assert got.ignored == want.ignored
    raw = ConfusionMatrix(C)                                          # no map: the values are the classes
    for k in range(VIEWS):
        raw.add_view(r, lcams[k], labels, mapped[k].astype(np.int16) if k % 2 else mapped[k], gt_undistort=True)
    np.testing.assert_array_equal(raw.get(), want.get())
    assert raw.ignored == want.ignored
    with pytest.raises(ValueError):
        got.add_views(r, lcams, labels, gts, gt_resize="nearest", gt_undistort=True)
    # colour ground truth: class = row of the palette, a colour outside it is ignored, and so are the pixels outside the sensor
    palette = rng.integers(0, 256, size=(C, 3)).astype(np.uint8)
    assert len({tuple(c) for c in palette}) == C and (1, 1, 1) not in {tuple(c) for c in palette}
    ids = [rng.integers(0, C + 3, size=(w, h)) for _ in range(VIEWS)]
    colours = [np.where((i < C)[:, :, None], palette[np.minimum(i, C - 1)], np.uint8(1)).astype(np.uint8) for i in ids]
    cplanes = [lr.ref_undistort_pixels(np.where(i < C, i, 255).astype(np.uint8), lens, view, 255)[0] for i, lens, view in zip(ids, lenses, views)]
    cwant, cgot = ConfusionMatrix(C), ConfusionMatrix(C)
    cwant.add_views(r, lcams, labels, cplanes)
    cgot.add_views(r, lcams, labels, colours, gt_palette=palette, gt_undistort=True)
    assert cwant.get().sum() > 0
    np.testing.assert_array_equal(cgot.get(), cwant.get())
    assert cgot.ignored == cwant.ignored


def test_refusals_the_zero_lens_and_plain_cameras(sm, oracle):
    C = 19
    mesh, cams, r, oidx, queued = scene(sm, oracle, "fine")
    lcams, lenses, views = lens_scene(sm, oracle)
    P = len(mesh.faces)
    small, big, wts = fusion_images(sm, oracle, C, "float32", SOURCES["full"])
    a = sm.fusion.MeshAggregator(P, C)
    a.fuse_view(r, lcams[0], small[0][0], undistort=True)
    before = bits(a.get_raw()).copy()
    assert before.any()
    for kwargs in ({"resize": "bilinear"}, {"resize": "bilinear", "sample_in_kernel": True}, {"sample_in_kernel": True}):
        with pytest.raises(ValueError, match="undistort"):
            a.fuse_views(r, lcams[:2], [small[0][0], small[1][0]], undistort=True, **kwargs)
        with pytest.raises(ValueError, match="undistort"):
            a.fuse_view(r, lcams[1], small[1][0], undistort=True, **kwargs)
    for call in (a.fuse_views_labels, ):
        with pytest.raises(ValueError, match="undistort"):
            call(r, lcams[:1], [np.zeros((W, H), np.uint8)], undistort=True, resize="nearest")
    with pytest.raises(ValueError, match="undistort"):
        a.fuse_view_labels(r, lcams[0], np.zeros((W, H), np.uint8), undistort=True, resize="nearest")
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        sm.data.LensCamera(cams[0].rotation, cams[0].translation, np.array([W, H]), cams[0].focal_lengths, cams[0].principal_point,
                           "OPENCV_FISHEYE", [0.1, 0.0, 0.0, 0.0])
    assert not a._pending
    np.testing.assert_array_equal(bits(a.get_raw()), before)
    # the zero lens through its default view at the image's size: the plain call in bits, and no kernel of lens.hip is launched
    zeros = [sm.data.LensCamera(c.rotation, c.translation, np.array([W, H]), c.focal_lengths, c.principal_point, "OPENCV", [0.0] * 4)
             for c in cams[:VIEWS]]
    plain = sm.fusion.MeshAggregator(P, C)
    plain.fuse_views(r, cams[:VIEWS], [v for v, _ in small])
    launches = sm._lib.get_option("lens_launches")
    z = sm.fusion.MeshAggregator(P, C)
    z.fuse_views(r, zeros, [v for v, _ in small], undistort=True)
    assert sm._lib.get_option("lens_launches") == launches
    np.testing.assert_array_equal(bits(z.get_raw()), bits(plain.get_raw()))
    # plain Cameras inside a batch pass through untouched: their images are the view's already
    mixed_cams = [cams[k] if k in (2, 3, 9) else lcams[k] for k in range(VIEWS)]
    mixed_imgs = [big[k] if k in (2, 3, 9) else small[k][0] for k in range(VIEWS)]
    m = sm.fusion.MeshAggregator(P, C)
    m.fuse_views(r, mixed_cams, mixed_imgs, undistort=True)
    assert sm._lib.get_option("lens_launches") == launches + VIEWS - 3
    full_wts = [None if k in (2, 3, 9) else wts[k] for k in range(VIEWS)]
    want = oracle_raw(oracle, P, C, "sum", 0.5, oidx[:VIEWS], big, weights=[np.ones((W, H), np.float32) if x is None else x for x in full_wts])[0]
    np.testing.assert_array_equal(bits(m.get_raw()), bits(want))
    # an undistorting fuse_view first hands over the views already deferred
    from semantic_meshes_amd.device import to_device
    order = sm.fusion.MeshAggregator(P, C)
    if order.defer:
        order.fuse_view(r, cams[2], to_device(big[2]))
        assert len(order._pending) == 1
        order.fuse_view(r, lcams[0], small[0][0], undistort=True)
        assert not order._pending
