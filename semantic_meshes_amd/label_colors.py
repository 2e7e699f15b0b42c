"""Label images that are COLOUR images (include/smesh_label_colors.h): the distinct colours of images on the device
(`unique_colors`), a palette given beforehand (`ColorTable`) and one discovered as the images arrive (`ColorRemap`, what the
reference's python/scripts/colorize_mesh.py --remap builds per frame on the host).  The `palette=` keyword of the label entry points
(fusion.py) and `gt_palette=` of the confusion matrices (evaluation.py) take them.  `fusion` re-exports the names.

A colour image is (w,h,3) or (w,h,4) uint8 -- a decoded (H,W,3) array is passed as its `transpose(1, 0, 2)` view --; alpha is
ignored; key = r << 16 | g << 8 | b, so ascending keys are np.unique(rows, axis=0)'s order."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, describe, release_to

FIRST_CAP = 4096        # keys per image asked for first by unique_colors; an image with more is asked again with its count


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def color_keys(colors):
    """(K,3) uint8 colours -> uint32 keys r << 16 | g << 8 | b."""
    c = np.asarray(colors)
    if c.ndim != 2 or c.shape[1] != 3 or c.dtype != np.uint8:
        raise ValueError("colours must be a (K,3) uint8 array, got %s %s" % (c.dtype, c.shape))
    c = c.astype(np.uint32)
    return (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]


def key_colors(keys):
    """uint32 keys -> (K,3) uint8 colours."""
    k = np.asarray(keys, dtype=np.uint32)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=-1).astype(np.uint8).reshape(-1, 3)


class ColorTable:
    """A known palette: `colors` (K,3) uint8, `classes` an integer [K] array (default: the row index, which is what `LabelRenderer`
    takes as its palette).  Kept sorted by key, as the library wants it.  Two equal colours with different classes are refused; with
    the same class they collapse into one entry.  A class outside [0, classes of the aggregator) makes its colour don't care."""

    def __init__(self, colors, classes=None):
        keys = color_keys(colors)
        if len(keys) == 0:
            raise ValueError("a colour table needs at least one colour")
        if classes is None:
            cls = np.arange(len(keys), dtype=np.int64)
        else:
            cls = np.asarray(classes)
            if cls.ndim != 1 or cls.dtype.kind not in "iu" or len(cls) != len(keys):
                raise ValueError("classes must be an integer array with one entry per colour, got %s %s for %d colours"
                                 % (cls.dtype, cls.shape, len(keys)))
            cls = cls.astype(np.int64)      # (a uint64 value beyond int64 wraps to a negative one: no class either)
        cls = np.where((cls > 0x7FFFFFFF) | (cls < 0), -1, cls)      # (what int32 cannot hold is no class of any aggregator)
        order = np.argsort(keys, kind="stable")
        keys, cls = keys[order], cls[order]
        same = np.concatenate([[False], keys[1:] == keys[:-1]])
        if (same & np.concatenate([[False], cls[1:] != cls[:-1]])).any():
            k = int(keys[np.nonzero(same & np.concatenate([[False], cls[1:] != cls[:-1]]))[0][0]])
            raise ValueError("colour (%d, %d, %d) is given two different classes" % (k >> 16, (k >> 8) & 255, k & 255))
        self.keys = np.ascontiguousarray(keys[~same], dtype=np.uint32)
        self.classes = np.ascontiguousarray(cls[~same], dtype=np.int32)

    def __len__(self):
        return len(self.keys)

    @property
    def colors(self):
        return key_colors(self.keys)

    def _args(self):
        """(keys pointer, classes pointer, K) for the C ABI."""
        return self.keys.ctypes.data_as(ctypes.c_void_p), self.classes.ctypes.data_as(ctypes.c_void_p), len(self.keys)


def _shape_of(image):
    return tuple(getattr(image, "shape", None) or np.shape(image))


def describe_color_source(image, device, streams, what="label image"):
    """(pointer, memkind, (w, h), dtype code, three element strides, keep-alive, channels) of a (w,h,3 or 4) uint8 colour image that
    the library is to look up: it goes over as it is."""
    lp, lmem, lshape, ldt, lstr, keep = describe(image, 3, what, device, streams)
    if ldt != np.uint8 or lshape[2] not in (3, 4):
        raise ValueError("%s: a colour image is (w,h,3) or (w,h,4) uint8, got %s %s" % (what, ldt, tuple(lshape)))
    return lp, lmem, (int(lshape[0]), int(lshape[1])), _lib.LBL_CODES["uint8"], tuple(int(s) for s in lstr), keep, int(lshape[2])


def _describe_any(image, device, streams, what):
    """describe_color_source's tuple for a colour image or a 2-D uint8 / uint16 one (channels = 1)."""
    nd = len(_shape_of(image))
    if nd == 3:
        return describe_color_source(image, device, streams, what)
    if nd != 2:
        raise ValueError("%s must be (w,h,3), (w,h,4) or (w,h), got shape %s" % (what, _shape_of(image)))
    lp, lmem, lshape, ldt, lstr, keep = describe(image, 2, what, device, streams)
    if ldt.name not in ("uint8", "uint16"):
        raise ValueError("%s: a one-channel image of colours is uint8 or uint16, got %s" % (what, ldt))
    return lp, lmem, (int(lshape[0]), int(lshape[1])), _lib.LBL_CODES[ldt.name], (int(lstr[0]), int(lstr[1]), 1), keep, 1


def unique_keys(images, device=0):
    """The ascending uint32 keys of every image of the list, and their channel counts (1 or 3; 4 counts as 3): consecutive images of
    one shape, dtype, layout and memory go to `smesh_colors_unique` together, which works them off in groups of eight."""
    images = list(images)
    streams = []
    desc = [_describe_any(im, int(device), streams, "image %d" % i) for i, im in enumerate(images)]
    out = [None] * len(images)
    lib = _lib.lib()
    start = 0
    for i in range(1, len(desc) + 1):
        if i < len(desc) and desc[i][1:5] == desc[start][1:5] and desc[i][6] == desc[start][6]:
            continue
        run, first = desc[start:i], desc[start]
        n = len(run)
        ptrs = (ctypes.c_void_p * n)(*[d[0] for d in run])
        counts = np.zeros(n, np.uint64)
        cap = FIRST_CAP
        while True:
            keys = np.empty((n, cap), np.uint32)
            _lib.check(lib.smesh_colors_unique(ptrs, n, first[6], first[3], _c64(first[4]), first[1], first[2][0], first[2][1],
                                               keys.ctypes.data_as(ctypes.c_void_p), cap, counts.ctypes.data_as(ctypes.c_void_p), int(device)))
            if int(counts.max()) <= cap:
                break
            cap = int(counts.max())      # (the true counts: the second request is the last)
        for j in range(n):
            out[start + j] = keys[j, :int(counts[j])].copy()
        start = i
    release_to(int(device), streams)
    return out, [1 if d[6] == 1 else 3 for d in desc]


def unique_colors(image, device=0):
    """The distinct colours of `image` -- (w,h,3) / (w,h,4) uint8, or (w,h) uint8 / uint16; host numpy or device array, any
    non-negative strides --, found on the device: (K,3) uint8 in ascending row order, what
    `np.unique(image.reshape(-1, ch)[:, :3], axis=0)` returns, or (K,) of the image's dtype for a 2-D image."""
    if isinstance(image, DeviceArray):
        device = image.device
    (keys,), (ch,) = unique_keys([image], device)
    if ch == 1:
        dt = getattr(image, "dtype", None)
        return keys.astype(np.asarray(image).dtype if dt is None else np.dtype(dt))
    return key_colors(keys)


class ColorRemap:
    """The growing dictionary colour -> class of colorize_mesh.py --remap: it starts empty; for each image, in the caller's order, the
    image's distinct colours are visited in ascending key order, and a colour not yet in the dictionary gets class `len(dictionary)`.
    The channel count (1: a 2-D image, key = value; 3: colour images, a fourth channel is ignored) is fixed by the first image.  The
    distinct colours are found on the device (`smesh_colors_unique`); only they cross PCIe.  A remap has no class limit of its own."""

    def __init__(self):
        self.color_to_class = {}      # tuples (r, g, b) or (v,), like the script's
        self.channels = None
        self._keys = {}               # key -> class

    def __len__(self):
        return len(self._keys)

    def update(self, images, device=0):
        """Take in one image or a list of images, host or device."""
        if isinstance(images, (np.ndarray, DeviceArray)) or hasattr(images, "__cuda_array_interface__") or hasattr(images, "__dlpack__"):
            images = [images]
        images = list(images)
        for im in images:
            if isinstance(im, DeviceArray):
                device = im.device
                break
        nds = [1 if len(_shape_of(im)) == 2 else 3 for im in images]
        want = self.channels if self.channels is not None else (nds[0] if nds else None)
        if any(c != want for c in nds):
            raise ValueError("a ColorRemap takes images of one channel count: %s, then %s" % (want, [c for c in nds if c != want][0]))
        keys, chans = unique_keys(images, device)
        if images and self.channels is None:
            self.channels = chans[0]
        for ks in keys:
            for k in ks.tolist():
                if k not in self._keys:
                    c = len(self._keys)
                    self._keys[k] = c
                    self.color_to_class[(k >> 16, (k >> 8) & 255, k & 255) if self.channels == 3 else (k,)] = c
        return self

    def class_to_color(self, classes):
        """uint8 [classes, 3]: the colour of every class, all-zero rows for classes no colour has (a one-channel colour v is
        (v, v, v)); the inverse table the script builds at its end, and a palette for `LabelRenderer`."""
        out = np.zeros((int(classes), 3), np.int64)
        for color, c in self.color_to_class.items():
            if c < int(classes):
                out[c] = color if len(color) == 3 else (color[0],) * 3
        return out.astype(np.uint8)

    def table(self):
        """The dictionary as the library takes it: a `ColorTable` (3 channels), or a one-dimensional `label_map` (1 channel)."""
        if not self._keys:
            raise ValueError("the ColorRemap has seen no colour yet")
        keys = np.fromiter(self._keys.keys(), np.int64, len(self._keys))
        cls = np.fromiter(self._keys.values(), np.int64, len(self._keys))
        if self.channels == 1:
            m = np.full(int(keys.max()) + 1, -1, np.int32)
            m[keys] = cls
            return m
        return ColorTable(key_colors(keys), cls)


def check_palette(palette, label_map=None, remap_ok=True, what="palette"):
    """The `palette=` keyword: None, a `ColorTable`, a `ColorRemap` (where `remap_ok`), or a (K,3) uint8 array (class = row index)."""
    if palette is None:
        return None
    if label_map is not None:
        raise ValueError("%s= and label_map= exclude each other: a colour image has no integer ids to map" % what)
    if isinstance(palette, ColorTable):
        return palette
    if isinstance(palette, ColorRemap):
        if not remap_ok:
            raise ValueError("%s= takes an array or a ColorTable, not a ColorRemap: ground truth has a known palette" % what)
        return palette
    return ColorTable(palette)


def resolve_palette(pal, images, classes, device):
    """What a call with `palette=pal` hands to the library: (colour table or None, label map or None).  A `ColorRemap` is first
    updated with the call's images, in their order; holding more colours than `classes` afterwards is the script's
    `assert mask < classes`: a ValueError before anything is fused (the remap keeps what it has seen)."""
    if not isinstance(pal, ColorRemap):
        return pal, None
    pal.update(images, device)
    if len(pal) > int(classes):
        raise ValueError("the ColorRemap holds %d colours, more than the %d classes" % (len(pal), int(classes)))
    t = pal.table()
    return (t, None) if isinstance(t, ColorTable) else (None, t)
