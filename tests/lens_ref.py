"""numpy restatement of include/smesh_lens.h for the tests: the map from a pixel of the pinhole view to the source
image in float64, every operation rounded separately (numpy does not contract), the bilinear form with resize_ref's float32 lerps,
the nearest form, the weights plane and the counts.  It shares no code with the library; 16-bit images are widened and narrowed by
half_helpers.  A lens here is a dict: f (2), c (2), k (6), p (2), size (wc, hc); a view a dict: F (2), P (2), size (W, H)."""
import numpy as np

import half_helpers as hh
from resize_ref import lerp

# model -> (slots of k1 .. k6 the model's distortion parameters fill, slots of p1, p2), in COLMAP's parameter order after f and c
SLOTS = {
    "SIMPLE_RADIAL": ((0,), ()),                       # k
    "RADIAL": ((0, 1), ()),                            # k1 k2
    "OPENCV": ((0, 1), (0, 1)),                        # k1 k2 p1 p2
    "FULL_OPENCV": ((0, 1, 2, 3, 4, 5), (0, 1)),       # k1 k2 p1 p2 k3 k4 k5 k6
}


def distortion_params(model, k, p=()):
    """The model's distortion parameters in COLMAP's order from its k's and p's."""
    k, p = list(k), list(p)
    return k[:2] + p + k[2:] if model in ("OPENCV", "FULL_OPENCV") else k


def make_lens(model, f, c, k, p, size):
    kk, pp = np.zeros(6), np.zeros(2)
    kk[:len(k)] = k
    pp[:len(p)] = p
    assert len(k) == len(SLOTS[model][0]) and len(p) == len(SLOTS[model][1])
    return dict(model=model, f=np.asarray(f, np.float64), c=np.asarray(c, np.float64), k=kk, p=pp, size=(int(size[0]), int(size[1])))


def make_view(F, P, size):
    """The view as the library holds it: a Camera rounds F and P to float32."""
    r = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    return dict(F=r(F), P=r(P), size=(int(size[0]), int(size[1])))


def lens_map(lens, view, w, h, X=None, Y=None):
    """(tx, ty, inside) of output pixels (X, Y) -- default: the whole (W,H) grid -- for a (w,h) source image."""
    W, H = view["size"]
    if X is None:
        X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    k1, k2, k3, k4, k5, k6 = (np.float64(v) for v in lens["k"])
    p1, p2 = (np.float64(v) for v in lens["p"])
    with np.errstate(all="ignore"):
        x = ((X + 0.5) - view["P"][0]) / view["F"][0]
        y = ((Y + 0.5) - view["P"][1]) / view["F"][1]
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        n = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        d = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
        s = n / d
        dx = (2.0 * p1) * xy + p2 * (r2 + 2.0 * xx)
        dy = p1 * (r2 + 2.0 * yy) + (2.0 * p2) * xy
        xd, yd = x * s + dx, y * s + dy
        u, v = lens["f"][0] * xd + lens["c"][0], lens["f"][1] * yd + lens["c"][1]
        tx = u * (np.float64(w) / np.float64(lens["size"][0])) - 0.5
        ty = v * (np.float64(h) / np.float64(lens["size"][1])) - 0.5
        inside = (d > 0) & (-0.5 <= tx) & (tx <= w - 0.5) & (-0.5 <= ty) & (ty <= h - 0.5)
    return tx, ty, inside


def _axis(t, n):
    t = np.minimum(np.maximum(t, 0.0), np.float64(n - 1))
    i0 = np.floor(t)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0.astype(np.int64), i1.astype(np.int64), (t - i0).astype(np.float32)


def ref_undistort_probs(src, lens, view):
    """float32 (w,h,C) -> (float32 (W,H,C), inside bool (W,H)); outside rows are +0.0."""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 3
    w, h, C = src.shape
    tx, ty, inside = lens_map(lens, view, w, h)
    tx, ty = np.where(inside, tx, 0.0), np.where(inside, ty, 0.0)
    x0, x1, fx = _axis(tx, w)
    y0, y1, fy = _axis(ty, h)
    fx, fy = fx[:, :, None], fy[:, :, None]
    top = lerp(src[x0, y0], src[x1, y0], fx)
    bot = lerp(src[x0, y1], src[x1, y1], fx)
    out = lerp(top, bot, fy)
    out[~inside] = np.float32(0.0)
    return out, inside


def ref_undistort_probs_as(src_wide, lens, view, out_dtype):
    """What the library hands back for `out_dtype`: float32 values, or uint16 bit patterns narrowed to nearest even."""
    out, inside = ref_undistort_probs(src_wide, lens, view)
    return (out if out_dtype == "float32" else hh.narrow(out, out_dtype)), inside


def ref_undistort_pixels(src, lens, view, fill):
    """(w,h[,ch]) of any dtype -> ((W,H[,ch]), inside): nearest, `fill` outside."""
    src = np.asarray(src)
    w, h = src.shape[:2]
    tx, ty, inside = lens_map(lens, view, w, h)
    tx, ty = np.where(inside, tx, 0.0), np.where(inside, ty, 0.0)
    ix = np.minimum(np.maximum(np.floor(tx + 0.5), 0), w - 1).astype(np.int64)
    iy = np.minimum(np.maximum(np.floor(ty + 0.5), 0), h - 1).astype(np.int64)
    out = src[ix, iy].copy()
    out[~inside] = np.asarray(fill, src.dtype)
    return out, inside


def ref_weights(inside, weights_image=None):
    """inside ? w_in : 0, float32 (W,H)."""
    w_in = np.ones(inside.shape, np.float32) if weights_image is None else np.asarray(weights_image, np.float32)
    return np.where(inside, w_in, np.float32(0.0)).astype(np.float32)


def ref_counts(inside):
    return np.array([inside.size, int((~inside).sum())], np.uint64)


def colmap_project(model, f, c, params, point):
    """COLMAP's forward projection of a 3-D point in the camera frame to calibration pixels, scalar and written on its own (from
    COLMAP's documentation of the models, not from the rule above): the check that the rule is applied in the right direction."""
    X, Y, Z = (float(v) for v in point)
    u, v = X / Z, Y / Z
    r2 = u * u + v * v
    if model == "SIMPLE_RADIAL":
        (k,) = params
        radial = k * r2
        du, dv = u * radial, v * radial
    elif model == "RADIAL":
        k1, k2 = params
        radial = k1 * r2 + k2 * r2 * r2
        du, dv = u * radial, v * radial
    elif model == "OPENCV":
        k1, k2, p1, p2 = params
        radial = k1 * r2 + k2 * r2 * r2
        du = u * radial + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
        dv = v * radial + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    elif model == "FULL_OPENCV":
        k1, k2, p1, p2, k3, k4, k5, k6 = params
        radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        du = u * radial - u + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
        dv = v * radial - v + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    else:
        raise ValueError(model)
    return f[0] * (u + du) + c[0], f[1] * (v + dv) + c[1]


# The lenses of the tests: f = (0.8 wc, 0.82 wc), c = (wc / 2 + 1.3, hc / 2 - 0.7)
TEST_LENSES = (("SIMPLE_RADIAL", (-0.12,), ()), ("SIMPLE_RADIAL", (0.15,), ()), ("RADIAL", (-0.2, 0.05), ()),
               ("OPENCV", (-0.25, 0.08), (0.01, -0.008)), ("FULL_OPENCV", (0.3, -0.1, 0.02, 0.5, -0.05, 0.01), (0.002, 0.003)))


def test_lens(index, wc, hc):
    model, k, p = TEST_LENSES[index]
    return make_lens(model, (0.8 * wc, 0.82 * wc), (wc / 2 + 1.3, hc / 2 - 0.7), k, p, (wc, hc))


test_lens.__test__ = False      # (not a test: pytest collects test_* callables of test modules that import it by name)


def default_view(lens):
    return make_view(lens["f"], lens["c"], lens["size"])
