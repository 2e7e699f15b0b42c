"""numpy restatement of include/smesh_label_prep.h: the sampling rule, the map and the narrowing, and the wrong rules the tests'
inputs must be able to tell from it.  Shared by test_label_prep_host.py and test_gpu_label_prep.py; nothing here touches the product."""
import numpy as np

import sampled_inputs as si

# source sizes of the fusion tests, for views of 160 x 120: sampled_inputs.SOURCES, and a ratio of 2.5 -- "half" is an exact doubling,
# where floor(X n / N) and the rule coincide, so it cannot tell the legacy rule from the right one (test_label_prep_host.py)
FUSION_SOURCES = dict(si.SOURCES, **{"0.4": (64, 48)})

# what resize_ref.SHAPES lacks: partial tiles on both axes, more than one 64 x 64 tile, and the same pair downscaling
EXTRA_SHAPES = (((130, 67), (300, 150)), ((300, 150), (130, 67)))


def axis_index(n, N):
    """The rule, one axis: i = ((2X + 1) n) div (2N) for X in [0, N), in Python-exact int64."""
    X = np.arange(N, dtype=np.int64)
    return ((2 * X + 1) * np.int64(n)) // np.int64(2 * N)


def legacy_axis_index(n, N):
    """torch's legacy mode="nearest": floor(X n / N).  NOT the rule."""
    return (np.arange(N, dtype=np.int64) * np.int64(n)) // np.int64(N)


def as_int64(values):
    """Any accepted label dtype as int64; a uint64 value int64 cannot hold is no class and no map index: -1."""
    a = np.asarray(values)
    out = a.astype(np.int64)
    if a.dtype == np.uint64:
        out[a > np.uint64(2 ** 63 - 1)] = -1
    return out


def sample(src, W, H, rule=axis_index):
    """(w,h) -> (W,H), int64."""
    a = as_int64(src)
    w, h = a.shape
    return a[rule(w, W)[:, None], rule(h, H)[None, :]]


def apply_map(values, label_map):
    """v in [0, M) -> map[v]; everything else -> -1 (don't care)."""
    v = np.asarray(values, dtype=np.int64)
    m = np.asarray(label_map).astype(np.int64)
    ok = (v >= 0) & (v < len(m))
    return np.where(ok, m[np.where(ok, v, 0)], -1)


def narrow(values, C):
    """int64 values -> the plane: uint8 up to 255 classes, else uint16; outside [0, C): all ones."""
    v = np.asarray(values, dtype=np.int64)
    dt = np.uint8 if C <= 255 else np.uint16
    return np.where((v >= 0) & (v < C), v, np.iinfo(dt).max).astype(dt)


def prepare(src, C, size=None, label_map=None, rule=axis_index):
    """What `prepare_labels(src, C, size, "nearest", label_map)` must return: sample, then map, then narrow."""
    src = np.asarray(src)
    W, H = src.shape if size is None else size
    v = sample(src, W, H, rule)
    if label_map is not None:
        v = apply_map(v, label_map)
    return narrow(v, C)


def make_map(rng, M, C):
    """A table of M entries that is no permutation: classes in [0, C) with repeats, about a tenth -1 and a tenth >= C."""
    m = rng.integers(0, C, size=M).astype(np.int32)
    u = rng.random(M)
    m[u < 0.1] = -1
    m[(u >= 0.1) & (u < 0.2)] = C + rng.integers(0, 3, size=int(((u >= 0.1) & (u < 0.2)).sum()))
    return m


def make_source(rng, w, h, dtype, top, bad=0.06):
    """(w,h) of `dtype`: values in [0, top) and, where the dtype can hold them, about `bad` of negative ones and ones >= top."""
    info = np.iinfo(dtype)
    v = rng.integers(0, max(min(top, info.max + 1), 1), size=(w, h)).astype(np.int64)
    out = rng.random((w, h)) < bad
    v[out] = rng.choice([-1, -7, top, top + 1, info.max], size=int(out.sum()))
    return np.clip(v, info.min, info.max).astype(dtype)
