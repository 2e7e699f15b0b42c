"""Cameras with lens distortion, without a GPU (include/smesh_lens.h): COLMAP workspaces with every polynomial model, the refusals,
and lens_ref.py -- the numpy restatement of DESIGN.md 3.18 that the GPU tests compare the kernels with -- checked on its own: against
a separately written COLMAP forward projection (a restatement that only agrees with the kernel cannot catch a model applied in the
wrong direction) and against validity counts worked out beforehand."""
import numpy as np
import pytest

import lens_ref as lr
import semantic_meshes_amd as sm

CAMERAS = """# Camera list with one line of data per camera:
1 SIMPLE_RADIAL 640 480 500 320 240 0.01
2 RADIAL 640 480 501 321 241 0.02 -0.03
3 OPENCV 640 480 502 503 322 242 0.04 -0.05 0.006 -0.007
4 FULL_OPENCV 640 480 504 505 323 243 0.08 -0.09 0.001 -0.002 0.03 0.4 -0.05 0.006
5 PINHOLE 640 480 506 507 324 244
6 OPENCV_FISHEYE 640 480 508 509 325 245 0.01 0.02 0.03 0.04
"""
IMAGES = "".join("%d 1 0 0 0 0.5 -0.25 2 %d %s.png\n\n" % (i, i, n) for i, n in enumerate("abcdef", 1))


@pytest.fixture()
def workspace(tmp_path):
    (tmp_path / "cameras.txt").write_text(CAMERAS)
    (tmp_path / "images.txt").write_text(IMAGES)
    return sm.data.Colmap(str(tmp_path))


def test_every_polynomial_model_lands_in_its_slots(workspace):
    want = {
        "a.png": ("SIMPLE_RADIAL", (500, 500), (320, 240), (0.01, 0, 0, 0, 0, 0), (0, 0)),
        "b.png": ("RADIAL", (501, 501), (321, 241), (0.02, -0.03, 0, 0, 0, 0), (0, 0)),
        "c.png": ("OPENCV", (502, 503), (322, 242), (0.04, -0.05, 0, 0, 0, 0), (0.006, -0.007)),
        "d.png": ("FULL_OPENCV", (504, 505), (323, 243), (0.08, -0.09, 0.03, 0.4, -0.05, 0.006), (0.001, -0.002)),
    }
    for name, (model, f, c, k, p) in want.items():
        cam = workspace.getLensCamera(name)
        assert isinstance(cam, sm.data.LensCamera) and isinstance(cam, sm.data.Camera)
        lens = cam.lens
        assert lens.model == model and lens.resolution == (640, 480)
        assert lens.focal.tolist() == list(f) and lens.principal.tolist() == list(c)
        assert lens.k.tolist() == list(k) and lens.p.tolist() == list(p)
        pod = lens._pod
        assert list(pod.focal) == list(f) and list(pod.principal) == list(c) and list(pod.k) == list(k) and list(pod.p) == list(p)
        assert (pod.width, pod.height) == (640, 480)
        # the default view: the lens's own f, c and size, as a Camera holds them
        assert cam.resolution == (640, 480) and cam.default_view
        assert cam.focal_lengths.tolist() == list(f) and cam.principal_point.tolist() == list(c)
        np.testing.assert_array_equal(cam.translation, np.float32([0.5, -0.25, 2]))
    pin = workspace.getLensCamera("e.png")
    assert type(pin) is sm.data.Camera and pin.focal_lengths.tolist() == [506, 507]
    assert [type(c).__name__ for c in (workspace.getLensCamera(i) for i in range(5))] == ["LensCamera"] * 4 + ["Camera"]


def test_the_fisheye_model_is_refused_by_name(workspace):
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        workspace.getLensCamera("f.png")
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        workspace.getLensCameras()
    for model in ("OPENCV_FISHEYE", "FOV", "THIN_PRISM_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"):
        with pytest.raises(ValueError, match=model):
            sm.data.LensCamera(np.eye(3), np.zeros(3), [64, 48], [50.0, 50.0], [32.0, 24.0], model, [0.1])


def test_get_camera_still_refuses_every_lens_model(workspace):
    for name in "abcdf":
        with pytest.raises(ValueError):
            workspace.getCamera(name + ".png")
    assert workspace.getCamera("e.png").resolution == (640, 480)
    with pytest.raises(ValueError):
        workspace.getCameras()


def test_lens_camera_takes_distortion_parameters_or_the_whole_line():
    args = (np.eye(3), np.zeros(3), [64, 48], [51.0, 52.0], [33.0, 23.0])
    a = sm.data.LensCamera(*args, "OPENCV", [0.1, 0.2, 0.3, 0.4])
    b = sm.data.LensCamera(*args, "OPENCV", [51.0, 52.0, 33.0, 23.0, 0.1, 0.2, 0.3, 0.4])
    assert a.lens.k.tolist() == b.lens.k.tolist() == [0.1, 0.2, 0, 0, 0, 0] and a.lens.p.tolist() == b.lens.p.tolist() == [0.3, 0.4]
    with pytest.raises(ValueError):
        sm.data.LensCamera(*args, "OPENCV", [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        sm.data.LensCamera(*args, "OPENCV", [50.0, 52.0, 33.0, 23.0, 0.1, 0.2, 0.3, 0.4])      # another f than the argument
    with pytest.raises(ValueError):
        sm.data.LensCamera(*args, "RADIAL", [0.1, float("nan")])
    other = sm.data.LensCamera(*args, "RADIAL", [0.1, 0.2], view_focal_lengths=[45.0, 46.0], view_principal_point=[30.0, 20.0], view_resolution=[50, 40])
    assert other.resolution == (50, 40) and other.focal_lengths.tolist() == [45.0, 46.0] and not other.default_view
    assert other.lens.resolution == (64, 48) and other.lens.focal.tolist() == [51.0, 52.0]


VIEW_SIZES = ((64, 48), (67, 45), (130, 67))


@pytest.mark.parametrize("index", range(len(lr.TEST_LENSES)))
def test_the_restatement_goes_the_way_colmap_projects(index):
    """A 3-D point seen through the pinhole view lands on pixel (X, Y); seen through the lens it lands on (u, v) of the sensor.
    lens_map(X, Y) must be within one source pixel of (u, v)."""
    model, k, p = lr.TEST_LENSES[index]
    rng = np.random.default_rng(5 + index)
    for W, H in VIEW_SIZES:
        lens = lr.test_lens(index, W, H)
        views = [lr.default_view(lens), lr.make_view(0.9 * lens["f"], lens["c"] + np.array([2.5, -1.5]), (W, H))]
        for view in views:
            checked = 0
            while checked < 12:
                Z = rng.uniform(1.0, 5.0)
                point = np.array([rng.uniform(-0.3, 0.3) * Z, rng.uniform(-0.2, 0.2) * Z, Z])
                X = int(np.floor(view["F"][0] * point[0] / Z + view["P"][0]))
                Y = int(np.floor(view["F"][1] * point[1] / Z + view["P"][1]))
                if not (0 <= X < W and 0 <= Y < H):
                    continue
                centre = np.array([(X + 0.5 - view["P"][0]) / view["F"][0] * Z, (Y + 0.5 - view["P"][1]) / view["F"][1] * Z, Z])
                u, v = lr.colmap_project(model, lens["f"], lens["c"], lr.distortion_params(model, k, p), centre)
                for w, h in ((W, H), (W // 2, H // 2 + 1)):
                    tx, ty, inside = lr.lens_map(lens, view, w, h, X, Y)
                    su, sv = u * w / W - 0.5, v * h / H - 0.5
                    assert abs(tx - su) < 1e-9 * w and abs(ty - sv) < 1e-9 * h, (model, W, H, X, Y)
                    assert bool(inside) == (0 <= u <= W and 0 <= v <= H)
                # ... and the pixel the point itself falls on is within one source pixel of its own projection
                pu, pv = lr.colmap_project(model, lens["f"], lens["c"], lr.distortion_params(model, k, p), point)
                tx, ty, _ = lr.lens_map(lens, view, W, H, X, Y)
                assert abs(tx - (pu - 0.5)) <= 1.0 and abs(ty - (pv - 0.5)) <= 1.0, (model, W, H, X, Y)
                checked += 1


def test_the_validity_counts_of_the_test_lenses():
    """The +0.15 lens puts 313 of 3072, 303 of 3015 and 738 of 8710 pixels outside; the other four lenses none -- so the outside
    branch is covered on every shape and no lens leaves fewer than half its pixels inside."""
    want = {(64, 48): 313, (67, 45): 303, (130, 67): 738}
    for (W, H), outside in want.items():
        for index in range(len(lr.TEST_LENSES)):
            lens = lr.test_lens(index, W, H)
            for w, h in ((W, H), (W // 2, H // 2)):
                inside = lr.lens_map(lens, lr.default_view(lens), w, h)[2]
                assert lr.ref_counts(inside).tolist() == [W * H, outside if index == 1 else 0], (index, W, H, w, h)
                assert 2 * int(inside.sum()) >= W * H


def test_the_restatements_on_known_images():
    W, H = 64, 48
    lens = lr.test_lens(1, W, H)
    view = lr.default_view(lens)
    # a zero lens seen through its own view at its own size is the identity, NaN and infinities included
    zero = lr.make_lens("OPENCV", lens["f"], lens["c"], (0, 0), (0, 0), (W, H))
    zview = lr.make_view(zero["f"], zero["c"], (W, H))
    zero["f"], zero["c"] = zview["F"], zview["P"]      # (float32-exact, as a workspace with such values would give)
    rng = np.random.default_rng(1)
    src = rng.random((W, H, 3), dtype=np.float32)
    src[3, 4, 1], src[5, 6, 2] = np.nan, np.inf
    out, inside = lr.ref_undistort_probs(src, zero, zview)
    assert inside.all() and np.array_equal(out.view(np.uint32), src.view(np.uint32))
    mask = rng.integers(0, 40, (W, H)).astype(np.int16)
    got, _ = lr.ref_undistort_pixels(mask, zero, zview, -1)
    assert np.array_equal(got, mask)
    # a constant image stays constant inside and is +0.0 / the fill outside
    out, inside = lr.ref_undistort_probs(np.full((32, 24, 2), 0.25, np.float32), lens, view)
    assert (out[inside] == 0.25).all() and (out[~inside] == 0).all() and not np.signbit(out[~inside]).any()
    got, inside2 = lr.ref_undistort_pixels(np.full((32, 24), 7, np.uint8), lens, view, 255)
    assert np.array_equal(inside, inside2) and (got[inside] == 7).all() and (got[~inside] == 255).all()
    w_in = rng.random((W, H), dtype=np.float32)
    wts = lr.ref_weights(inside, w_in)
    assert np.array_equal(wts[inside], w_in[inside]) and (wts[~inside] == 0).all()
    assert np.array_equal(lr.ref_weights(inside), inside.astype(np.float32))
    # the +0.15 lens magnifies towards the border: the outside pixels are the border's
    assert not inside[0, 0] and not inside[W - 1, H - 1] and inside[W // 2, H // 2]


def test_the_plumbing_tables():
    from semantic_meshes_amd import _lib
    assert set(_lib.LENS_SIGNATURES) == {"smesh_undistort_probs", "smesh_undistort_pixels"}
    assert not set(_lib.LENS_SIGNATURES) & set(_lib.SIGNATURES)
    import ctypes
    assert ctypes.sizeof(_lib.LensPOD) == 12 * 8 + 16 and ctypes.sizeof(_lib.CameraPOD) == 96
    for name in ("undistort_probs_device", "undistort_labels_device", "undistort_depth_device", "undistort_probs", "undistort_labels",
                 "undistort_depth"):
        assert callable(getattr(sm.fusion, name))
