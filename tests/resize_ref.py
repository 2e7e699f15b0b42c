"""numpy restatement of include/smesh_resize.h for the tests: the axis tables in float64, the three float32 lerps with
the `f == 0` rule, and the test images.  16-bit images are widened and narrowed by half_helpers."""
import numpy as np

import half_helpers as hh

DTYPES = ("float32", "float16", "bfloat16")
# source (w,h) -> target (W,H): a 1 x 1 source, one-pixel axes, an exact doubling, odd ratios, the identity, downscaling, more than
# one workgroup per column and per image
SHAPES = (((1, 1), (6, 5)), ((1, 4), (3, 9)), ((4, 1), (9, 3)), ((4, 3), (8, 6)), ((5, 4), (13, 9)), ((7, 5), (7, 5)),
          ((13, 9), (5, 4)), ((40, 30), (81, 61)), ((37, 53), (130, 67)))


def axis_table(n, N):
    """(i0 int64[N], i1 int64[N], f float32[N]) of one axis: input size n, output size N.  IEEE double, every operation rounded
    separately (numpy does not contract)."""
    X = np.arange(N, dtype=np.float64)
    s = np.float64(n) / np.float64(N)
    t = (X + 0.5) * s - 0.5
    t = np.minimum(np.maximum(t, 0.0), np.float64(n - 1))
    i0 = np.floor(t)
    i1 = np.minimum(i0 + 1, n - 1)
    f = (t - i0).astype(np.float32)
    assert (f[i1 == i0] == 0).all()
    return i0.astype(np.int64), i1.astype(np.int64), f


def lerp(a, b, f):
    """(f == 0) ? a : a + (b - a) * f in float32, every operation rounded separately."""
    assert a.dtype == np.float32 and b.dtype == np.float32 and f.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        r = a + (b - a) * f
    assert r.dtype == np.float32
    return np.where(f == 0, a, r)


def ref_resize(src, W, H):
    """float32 (w,h,C) -> float32 (W,H,C)."""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 3
    w, h, C = src.shape
    x0, x1, fx = axis_table(w, W)
    y0, y1, fy = axis_table(h, H)
    fx, fy = fx[:, None, None], fy[None, :, None]
    top = lerp(src[x0][:, y0], src[x1][:, y0], fx)
    bot = lerp(src[x0][:, y1], src[x1][:, y1], fx)
    return lerp(top, bot, fy)


def ref_resize_as(src_wide, W, H, out_dtype):
    """What the library hands back for `out_dtype`: float32 values, or uint16 bit patterns narrowed to nearest even."""
    out = ref_resize(src_wide, W, H)
    return out if out_dtype == "float32" else hh.narrow(out, out_dtype)


def make_source(rng, w, h, C, dtype, special=False):
    """(values, widened): `values` (w,h,C) is what a user hands over -- float32, float16, or uint16 bits of bfloat16 -- and `widened`
    its exact float32 image.  Values in [0, 1) with every exponent down to binary16 subnormals; `special` plants NaN and both
    infinities."""
    p = (rng.random((w, h, C), dtype=np.float32) * np.float32(2.0) ** rng.integers(-26, 1, size=(w, h, C)).astype(np.float32)).astype(np.float32)
    if special:
        flat = p.reshape(-1)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            flat[(k * 7 + 1) % flat.size] = v
    if dtype == "float32":
        return p, p
    bits = hh.narrow(p, dtype)
    return hh.typed(bits, dtype), hh.widen(bits, dtype)


def widened(values, dtype):
    """The exact float32 image of what the library returned for `dtype`."""
    a = np.asarray(values)
    return a if dtype == "float32" else hh.widen(a.view(np.uint16), dtype)
