"""Inputs of the sample-in-kernel tests (include/smesh_sampled.h), shared by test_gpu_sampled.py and test_sampled_host.py: source
images at three sizes for views of 160 x 120, and what the fusion must see for each -- resize_ref.ref_resize of the widened source,
rounded to the source's dtype and widened again.  Everything is generated once per key and left unchanged."""
import numpy as np

import half_helpers as hh
import resize_ref as ref
from helpers import random_probs

W, H = 160, 120                      # test_gpu_half's scenes
# an exact halving; a non-integer ratio (fractional weights, clamped borders); a source larger than the view (downscaling)
SOURCES = {"half": (80, 60), "0.37": (59, 44), "down": (200, 150)}
DTYPES = ref.DTYPES
KINDS = ("sum", "summax")
IEWS = (0.0, 0.5, 1.0)               # image_equal_weight: 0 drops the image's weight out of a pixel's, 1 makes it all of it
_cache = {}


def main_cases():
    """(dtype, kind, C, size key, iew) of the bit-exact main-path test: every dtype x kind x class count x source size, the iew
    dealt round by the positions, so that each of the three values meets every (dtype, kind) pair, both class counts and every
    source size (test_sampled_host.py checks that it does)."""
    return [(dtype, kind, C, size, IEWS[(di + ki + ci + zi) % 3])
            for di, dtype in enumerate(DTYPES) for ki, kind in enumerate(KINDS)
            for ci, C in enumerate((19, 40)) for zi, size in enumerate(sorted(SOURCES))]


def seen(resampled, dtype):
    """What the fusion sees of a resampled float32 image: the image rounded to the source's dtype and widened again."""
    return resampled if dtype == "float32" else hh.widen(hh.narrow(resampled, dtype), dtype)


def source_images(C, dtype, size, n):
    """([(values, widened)] * n, [what the fusion must see] * n) for source images of `size` = (w,h).  About an eighth of the source
    pixels are all-zero don't-care rows, in runs along y, so that blended rows fall on both sides of the `sum > 0.5f` test in numbers;
    the 16-bit images are half_helpers.random_probs16's (rows scaled to just below and above 0.5, binary16 subnormals)."""
    key = ("src", C, dtype, size, n)
    if key not in _cache:
        w, h = size
        rng = np.random.default_rng(77 * C + 13 * w + 1000 * h + DTYPES.index(dtype))
        small, big = [], []
        for _ in range(n):
            holes = rng.random((w, h)) < 0.06
            holes |= np.roll(holes, 1, axis=1)                      # runs of two and more: whole blended rows of zeros, and halves
            if dtype == "float32":
                p = random_probs(rng, w, h, C)
                p[holes] = 0.0
                values = wide = p
            else:
                b = hh.random_probs16(rng, w, h, C, dtype)
                b[holes] = 0
                values, wide = hh.typed(b, dtype), hh.widen(b, dtype)
            small.append((values, wide))
            big.append(seen(ref.ref_resize(wide, W, H), dtype))
        _cache[key] = (small, big)
    return _cache[key]


def special_images(C, dtype, size, n):
    """`source_images` with NaN, both infinities, both zeros and (float16) subnormals planted, and all-zero pixels."""
    key = ("special", C, dtype, size, n)
    if key not in _cache:
        w, h = size
        small, _ = source_images(C, dtype, size, n)
        out_small, out_big = [], []
        for k, (_, wide0) in enumerate(small):
            wide = wide0.copy()
            flat = wide.reshape(-1)
            for j, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, 2.0 ** -20, 2.0 ** -24, -(2.0 ** -16))):
                flat[(j * 7919 + 31 * k + 5) % flat.size::max(flat.size // 9, 1)] = v
            wide[3::11, 2::7] = 0.0
            if dtype == "float32":
                values = wide
            else:
                bits = hh.narrow(wide, dtype)
                values, wide = hh.typed(bits, dtype), hh.widen(bits, dtype)
                if dtype == "float16":
                    assert hh.subnormal_f16(bits).any()
            with np.errstate(invalid="ignore"):
                out_small.append((values, wide))
                out_big.append(seen(ref.ref_resize(wide, W, H), dtype))
        _cache[key] = (out_small, out_big)
    return _cache[key]


def row_sums(img):
    """The float32 sequential sum of every pixel's row: what Mesh.h:98 compares with 0.5."""
    s = np.zeros(img.shape[:-1], np.float32)
    for c in range(img.shape[-1]):
        s = s + img[..., c]
    return s
