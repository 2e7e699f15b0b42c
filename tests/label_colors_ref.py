"""numpy restatement of include/smesh_label_colors.h: the key of a colour, the distinct colours of an image, the table lookup and the
growing remap, and the wrong rules the tests' inputs must be able to tell from it.  Shared by test_label_colors_host.py and
test_gpu_label_colors.py; nothing here touches the product."""
import numpy as np

import label_prep_ref as lp


def key_rgb(px):
    """THE rule: key = r << 16 | g << 8 | b of channels 0, 1, 2; a fourth channel is no part of it.  px: (..., 3 or 4) uint8."""
    p = np.asarray(px).astype(np.int64)
    return (p[..., 0] << 16) | (p[..., 1] << 8) | p[..., 2]


def key_bgr(px):
    """Channels in the order b, g, r.  NOT the rule."""
    p = np.asarray(px).astype(np.int64)
    return (p[..., 2] << 16) | (p[..., 1] << 8) | p[..., 0]


def key_with_alpha(px):
    """Alpha taken into the key.  NOT the rule."""
    p = np.asarray(px).astype(np.int64)
    k = key_rgb(p)
    return k if p.shape[-1] == 3 else (k << 8) | p[..., 3]


def keys_of(image, key=key_rgb):
    """The int64 key of every pixel of a (w,h,3), (w,h,4) or (w,h) image: a 2-D image's key is its value."""
    a = np.asarray(image)
    return a.astype(np.int64) if a.ndim == 2 else key(a)


def colors_of(keys):
    """Keys back to (K,3) uint8 rows."""
    k = np.asarray(keys, dtype=np.int64)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=-1).astype(np.uint8)


def unique_keys(image, key=key_rgb):
    """The distinct keys of an image, ascending."""
    return np.unique(keys_of(image, key))


def unique(image):
    """What `unique_colors(image)` must return: (K,3) uint8 rows in ascending order, or (K,) of the image's dtype for a 2-D image."""
    a = np.asarray(image)
    k = unique_keys(a)
    return k.astype(a.dtype) if a.ndim == 2 else colors_of(k)


def sort_table(colors, classes=None):
    """(keys ascending, classes) of a palette given as (K,3) rows; classes default to the row index."""
    keys = key_rgb(np.asarray(colors, dtype=np.uint8))
    cls = np.arange(len(keys), dtype=np.int64) if classes is None else np.asarray(classes, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    return keys[order], cls[order]


def lookup(keys, table_keys, table_classes):
    """A key that is table_keys[j] -> table_classes[j]; any other key -> -1 (don't care).  table_keys ascending."""
    k = np.asarray(keys, dtype=np.int64)
    tk, tc = np.asarray(table_keys, dtype=np.int64), np.asarray(table_classes, dtype=np.int64)
    j = np.clip(np.searchsorted(tk, k), 0, len(tk) - 1)
    return np.where(tk[j] == k, tc[j], -1)


def prepare(image, C, size, colors, classes=None, key=key_rgb):
    """What `prepare_labels(image, C, size, "nearest", palette=ColorTable(colors, classes))` must return: sample, then look up, then
    narrow.  (Sampling picks whole pixels, so sampling the keys is sampling the image.)"""
    tk, tc = sort_table(colors, classes)
    k = keys_of(image, key)
    W, H = k.shape if size is None else size
    return lp.narrow(lookup(lp.sample(k, W, H), tk, tc), C)


class Remap:
    """The growing dictionary: for each image in order, its distinct keys ascending; a new key gets class len(dictionary)."""

    def __init__(self):
        self.classes = {}      # key -> class

    def update(self, images):
        for im in images:
            for k in unique_keys(im).tolist():
                if k not in self.classes:
                    self.classes[k] = len(self.classes)
        return self

    def apply(self, image):
        """The image in classes, int64 (w,h)."""
        tk = np.array(sorted(self.classes), dtype=np.int64)
        return lookup(keys_of(image), tk, [self.classes[k] for k in tk.tolist()])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def make_palette(rng, K):
    """K distinct colours in random order, (K,3) uint8: keys spread over the whole range, 0 and 2^24 - 1 left out (the lookup tests
    use them as keys below the first and above the last entry)."""
    keys = np.unique(rng.integers(1, (1 << 24) - 1, size=2 * K + 16))      # (more than K distinct ones among them, for every K used)
    assert len(keys) >= K
    return colors_of(rng.permutation(keys)[:K])


def make_image(rng, w, h, colors, channels=3, absent=0.1):
    """(w,h,channels) uint8: pixels drawn from `colors` and, for about `absent` of them, from colours that are NOT among them: the keys
    next to present ones (key - 1, key + 1), key 0 and key 2^24 - 1 -- the bisection's off-by-one cases.  Alpha is random."""
    keys = key_rgb(colors)
    present = set(keys.tolist())
    near = np.concatenate([keys - 1, keys + 1, [0, (1 << 24) - 1]])
    near = np.array([k for k in near.tolist() if 0 <= k < (1 << 24) and k not in present] or [0], dtype=np.int64)
    k = keys[rng.integers(0, len(keys), size=(w, h))]
    out = rng.random((w, h)) < absent
    k[out] = near[rng.integers(0, len(near), size=int(out.sum()))]
    img = np.zeros((w, h, channels), np.uint8)
    img[..., :3] = colors_of(k)
    if channels == 4:
        img[..., 3] = rng.integers(0, 256, size=(w, h))
    return img


def layouts(src, device):
    """The (w,h[,ch]) image dense, as the transposed view of an (h,w[,ch]) array -- how a decoded image arrives --, and at strides
    larger than dense on both image axes; on the host or in device memory."""
    w, h = src.shape[:2]
    tail = src.shape[2:]
    tr = (1, 0) + ((2,) if tail else ())
    big = np.zeros((2 * w + 1, 3 * h + 2) + tail, src.dtype)
    big[1:1 + 2 * w:2, 2:2 + 3 * h:3] = src
    if not device:
        return {"dense": src, "transposed": np.ascontiguousarray(src.transpose(tr)).transpose(tr), "strided": big[1:1 + 2 * w:2, 2:2 + 3 * h:3]}
    from semantic_meshes_amd.device import DeviceArray, to_device
    dbig = to_device(big)
    ch = tail[0] if tail else 1
    pitch = big.shape[1] * ch
    strides = (2 * pitch, 3 * ch) + ((1,) if tail else ())
    return {"dense": to_device(src), "transposed": to_device(np.ascontiguousarray(src.transpose(tr))).transpose(*tr),
            "strided": DeviceArray(dbig.ptr + (pitch + 2 * ch) * src.dtype.itemsize, src.shape, src.dtype, dbig.device, strides, owner=dbig)}
