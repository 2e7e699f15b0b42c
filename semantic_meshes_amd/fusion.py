"""`semantic_meshes.fusion.MeshAggregator`.

Reference: /root/reference/python/semantic_meshes/src/Fusion.cu:120-150 (factory, defaults "sum", 0.5),
include/Fusion.h:42-76 (add1/add2/reset/get), /root/reference/include/semantic_meshes/fusion/Mesh.h:65-132.
The class count is a run-time value here (compile-time CLASSES_NUMS list in the reference).
"""
import ctypes
import threading

import numpy as np

from . import _lib
import os

from .device import DeviceArray, describe, release_to, result_empty

_IDX_CODES = {np.dtype(np.uint32): _lib.IDX_U32, np.dtype(np.int32): _lib.IDX_I32,
              np.dtype(np.uint64): _lib.IDX_U64, np.dtype(np.int64): _lib.IDX_I64}


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def narrow_labels(labels, classes):
    """The host-side narrowing rule of the label entry points: an integer label image (any of uint8 / int8 / uint16 / int16 / uint32 /
    int32 / uint64 / int64, any shape) as the dense plane the fusion reads -- uint8 when `classes` <= 255, else uint16 -- with every
    value outside [0, classes), negative ones included, replaced by the all-ones "don't care" code (255 / 65535: tf.one_hot's all-zero
    vector).  Only this plane crosses PCIe."""
    a = np.asarray(labels)
    classes = int(classes)
    if a.dtype.name not in _lib.LBL_CODES:
        raise ValueError("label image dtype must be one of %s, got %s" % ("/".join(_lib.LBL_CODES), a.dtype))
    if not 0 < classes <= 65535:
        raise ValueError("classes must be in [1, 65535]")
    out = np.dtype(np.uint8 if classes <= 255 else np.uint16)
    # one pass in the image's own width: seen as unsigned, a negative label is a huge one, so "outside [0, classes)" is `>= classes`
    u = a.view(np.dtype("u%d" % a.dtype.itemsize))
    limit = classes if a.dtype.kind == "u" else min(classes, np.iinfo(a.dtype).max + 1)
    code = np.iinfo(out).max
    if limit > np.iinfo(u.dtype).max:          # every value the image can hold is a class
        return np.ascontiguousarray(u.astype(out, copy=False))
    if out.itemsize > u.itemsize:              # (int8 labels, more than 255 classes: the code does not fit the image's width)
        return np.where(u < u.dtype.type(limit), u.astype(out), out.type(code))
    return np.ascontiguousarray(np.where(u < u.dtype.type(limit), u, u.dtype.type(code)).astype(out, copy=False))


def label_resize_mode(resize):
    """The `resize=` keyword of the LABEL entry points: None, or "nearest" -- nearest neighbour with half-pixel centres
    (include/smesh_label_prep.h).  Its own validation: the class-vector keyword (`resize.resize_mode`) knows "bilinear" only."""
    if resize is None:
        return None
    if resize == "bilinear":
        raise ValueError('resize="bilinear": label images are sampled, not blended -- use resize="nearest"')
    if resize != "nearest":
        raise ValueError('resize must be None or "nearest" for label images, got %r' % (resize,))
    return "nearest"


def check_label_map(label_map):
    """`label_map` of the label entry points as the library takes it: None, or a one-dimensional, non-empty integer table as a dense
    int32 array -- host numpy, or this library's own int32 DeviceArray as it is.  Source value v in [0, len) becomes map[v]; every
    other value is don't care, and so is every entry outside [0, classes)."""
    if label_map is None:
        return None
    if isinstance(label_map, DeviceArray):
        if label_map.ndim != 1 or label_map.dtype != np.int32 or (label_map.shape[0] > 1 and label_map.strides[0] != 1):
            raise ValueError("a label map on the device must be a dense one-dimensional int32 array, got %s %s" % (label_map.dtype, label_map.shape))
        m = label_map
    else:
        a = np.asarray(label_map)
        if a.ndim != 1:
            raise ValueError("label map must be one-dimensional, got shape %s" % (a.shape,))
        if a.dtype.kind not in "iu":
            raise ValueError("label map must be an integer table, got %s" % a.dtype)
        # (entries that int32 cannot hold are no class of any aggregator: -1 keeps them don't care)
        if a.size and a.dtype.itemsize >= 4:
            bad = (a > 0x7FFFFFFF) | (a < 0)
            a = a.astype(np.int64)
            a[bad] = -1
        m = np.ascontiguousarray(a, dtype=np.int32)
    if m.shape[0] == 0:
        raise ValueError("label map is empty")
    if m.shape[0] > 1 << 24:
        raise ValueError("label map has more than 2^24 entries")
    return m


def _map_args(m):
    """(pointer, length, memkind) of `check_label_map`'s result for the C ABI."""
    if m is None:
        return None, 0, _lib.MEM_HOST
    if isinstance(m, DeviceArray):
        return ctypes.c_void_p(m.ptr), int(m.shape[0]), _lib.MEM_DEVICE
    return m.ctypes.data_as(ctypes.c_void_p), int(m.shape[0]), _lib.MEM_HOST


def _describe_label_source(labels, device, streams, what="label image", m=None):
    """(pointer, memkind, (w, h), dtype code, element strides, keep-alive, channels) of a label image that the library is to prepare:
    it goes over as it is (the map sees the raw values).  A one-dimensional array is (n, 1).  With a `ColorTable` as `m` the image is
    a (w,h,3) / (w,h,4) colour image with three strides; else `channels` is 0."""
    if isinstance(m, ColorTable):
        return describe_color_source(labels, device, streams, what)
    if isinstance(labels, np.ndarray) and labels.ndim == 1:
        labels = labels.reshape(-1, 1)
    elif isinstance(labels, DeviceArray) and labels.ndim == 1:
        labels = DeviceArray(labels.ptr, (labels.shape[0], 1), labels.dtype, labels.device, (labels.strides[0], 1), owner=labels)
    lp, lmem, lshape, ldt, lstr, keep = describe(labels, 2, what, device, streams)
    if ldt.name not in _lib.LBL_CODES:
        raise ValueError("%s dtype must be one of %s, got %s" % (what, "/".join(_lib.LBL_CODES), ldt))
    return lp, lmem, (int(lshape[0]), int(lshape[1])), _lib.LBL_CODES[ldt.name], tuple(lstr), keep, 0


def _prepared_entry(name, m, w, h, channels):
    """(function, trailing arguments) of the entry point `name` that prepares label images: its `_colors` form (smesh_label_colors.h)
    for a `ColorTable`, else its `_prepared` form (smesh_label_prep.h) for `check_label_map`'s result."""
    if isinstance(m, ColorTable):
        return getattr(_lib.lib(), name + "_colors"), (w, h, channels) + m._args()
    return getattr(_lib.lib(), name + "_prepared"), (w, h) + _map_args(m)


def _palette_or_map(palette, label_map, images, classes, device):
    """`palette=` and `label_map=` of a label entry point as ONE value for the code below: None, `check_label_map`'s result, or a
    `ColorTable`.  A `ColorRemap` is first updated with the call's images (label_colors.resolve_palette) and then stands for its
    table -- for 2-D masks a label map, key = value."""
    m = check_label_map(label_map)
    pal = check_palette(palette, m)
    if pal is None:
        return m
    table, remapped = resolve_palette(pal, images, classes, device)
    return table if table is not None else check_label_map(remapped)


def prepare_labels_device(labels, classes, size=None, resize=None, label_map=None, device=0, palette=None):
    """The dense (W,H) plane the label fusion and the confusion matrices read, built ON THE DEVICE from a label image at its own
    resolution and in the dataset's ids (`smesh_labels_prepare`, include/smesh_label_prep.h): `labels` integer (w,h), host numpy or
    device array, any non-negative strides; `size` = (W,H), None: the image's own; `resize="nearest"` samples a (w,h) != (W,H) image
    with half-pixel centres (without it such a pair is refused); `label_map`, a one-dimensional integer table, turns source value v
    into map[v] AFTER sampling (v outside the table: don't care).  Every value outside [0, classes) becomes the all-ones code.
    `palette` (instead of `label_map`): `labels` is a (w,h,3) / (w,h,4) uint8 COLOUR image and a pixel gets the class of its colour
    -- a (K,3) uint8 array (class = row), a `ColorTable`, or a `ColorRemap`, which is first updated with this image and also takes a
    2-D mask (`smesh_labels_prepare_colors`, include/smesh_label_colors.h); a colour outside the palette is don't care.
    Returns a `DeviceArray`, uint8 for up to 255 classes, else uint16."""
    from .device import DeviceBuffer
    mode = label_resize_mode(resize)
    classes = int(classes)
    if not 0 < classes <= 65535:
        raise ValueError("classes must be in [1, 65535]")
    if isinstance(labels, DeviceArray):
        device = labels.device
    m = _palette_or_map(palette, label_map, [labels], classes, int(device))
    streams = []
    lp, lmem, (w, h), lcode, lstr, keep, ch = _describe_label_source(labels, int(device), streams, m=m)
    W, H = (w, h) if size is None else (int(size[0]), int(size[1]))
    if (W, H) != (w, h) and mode is None:
        raise ValueError('label image is %s, the target %s: pass resize="nearest" to sample it' % ((w, h), (W, H)))
    if W and H and not (w and h):
        raise ValueError("an empty label image %s cannot be resampled to %s" % ((w, h), (W, H)))
    dt = np.dtype(np.uint8 if classes <= 255 else np.uint16)
    out = DeviceBuffer(max(W * H * dt.itemsize, 1), int(device)).view((W, H), dt)
    if isinstance(m, ColorTable):
        kp, cp, K = m._args()
        _lib.check(_lib.lib().smesh_labels_prepare_colors(ctypes.c_void_p(lp), ch, _c64(lstr), lmem, w, h, kp, cp, K, classes,
                                                          ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], W, H, int(device)))
    else:
        mp, mlen, mmem = _map_args(m)
        _lib.check(_lib.lib().smesh_labels_prepare(ctypes.c_void_p(lp), lcode, _c64(lstr), lmem, w, h, mp, mlen, mmem, classes,
                                                   ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], W, H, int(device)))
    release_to(int(device), streams)
    return out


def prepare_labels(labels, classes, size=None, resize=None, label_map=None, device=0, palette=None):
    """`prepare_labels_device` copied to the host: a numpy array."""
    return prepare_labels_device(labels, classes, size, resize, label_map, device, palette).numpy()


def probs_code(dtype, keep=None, probs_dtype=None, what="probs image"):
    """The SMESH_PROBS_* code (include/smesh_half.h) of a class-vector image of numpy dtype `dtype`, or None for a dtype the fusion
    does not read.  float16 is recognised from the dtype.  numpy has no bfloat16: it is a dtype NAMED bfloat16 (ml_dtypes) where one
    is installed, a uint16 array that says so itself (`keep.bfloat16`: a DLPack import of kDLBfloat/16, `narrow_probs`' result), or a
    uint16 array with `probs_dtype="bfloat16"` -- its bits are bfloat16.  `probs_dtype` None: infer."""
    dtype = np.dtype(dtype)
    if probs_dtype is not None:
        name = probs_dtype if isinstance(probs_dtype, str) else np.dtype(probs_dtype).name
        if name == "bfloat16":
            if dtype == np.uint16 or (dtype.name == "bfloat16" and dtype.itemsize == 2):
                return _lib.PROBS_BF16
            raise ValueError('%s: probs_dtype="bfloat16" needs a uint16 array (its bits are bfloat16), got %s' % (what, dtype))
        if name not in ("float16", "float32"):
            raise ValueError("probs_dtype must be None, 'float32', 'float16' or 'bfloat16', got %r" % (probs_dtype,))
        if dtype.name != name and not (name == "float32" and dtype.kind == "f" and dtype.itemsize > 4):
            raise ValueError("%s: probs_dtype=%r but the array is %s" % (what, name, dtype))
    if dtype == np.float32:
        return _lib.PROBS_F32
    if dtype == np.float16:
        return _lib.PROBS_F16
    if (dtype.name == "bfloat16" and dtype.itemsize == 2) or (dtype == np.uint16 and getattr(keep, "bfloat16", False)):
        return _lib.PROBS_BF16
    return None


def _peek_code(obj, probs_dtype):
    """`probs_code` of an image without touching it (no copy, no stream ordering, no capsule consumed): None where that cannot be
    told from the outside."""
    dt = None
    if isinstance(obj, (np.ndarray, DeviceArray)):
        dt = obj.dtype
    else:
        try:
            cai = getattr(obj, "__cuda_array_interface__", None)
        except (TypeError, RuntimeError):
            cai = None
        if cai is not None:
            dt = np.dtype(cai["typestr"])
    if dt is None:
        return None
    return probs_code(dt, obj, probs_dtype)


def narrow_probs(array, dtype, device=0):
    """float32 class vectors rounded to float16 or bfloat16 ON THE DEVICE (`smesh_narrow_probs`: round to nearest even, overflow to
    inf, subnormals kept): a dense `DeviceArray` of the same shape in a fresh allocation -- float16, or uint16 bit patterns with
    `.bfloat16` set.  `array`: a float32 numpy array or dense float32 device array; `dtype`: "float16" / np.float16 / "bfloat16".
    For tests, benchmarks and users whose network ran in float32."""
    from .device import DeviceBuffer, to_device
    name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
    if name not in ("float16", "bfloat16"):
        raise ValueError("narrow_probs: dtype must be float16 or bfloat16, got %r" % (dtype,))
    if isinstance(array, np.ndarray) or not (isinstance(array, DeviceArray) or hasattr(array, "__cuda_array_interface__")):
        array = to_device(np.ascontiguousarray(array, dtype=np.float32), device)
    streams = []
    ptr, mem, shape, dt, strides, keep = describe(array, len(array.shape), "narrow_probs input", getattr(array, "device", device), streams)
    dev = int(getattr(array, "device", device)) if isinstance(array, DeviceArray) else int(device)
    dense = DeviceArray(0, shape, np.float32, dev).strides
    if dt != np.float32 or mem != _lib.MEM_DEVICE or tuple(strides) != tuple(dense):
        raise ValueError("narrow_probs needs a dense float32 array")
    n = 1
    for s in shape:
        n *= int(s)
    out = DeviceBuffer(max(n * 2, 2), dev).view(shape, np.float16 if name == "float16" else np.uint16)
    out.bfloat16 = name == "bfloat16"
    if n:
        _lib.check(_lib.lib().smesh_narrow_probs(ctypes.c_void_p(ptr), ctypes.c_void_p(out.ptr), n,
                                                 _lib.PROBS_F16 if name == "float16" else _lib.PROBS_BF16, dev, _lib.MEM_DEVICE))
    release_to(dev, streams)
    if not isinstance(keep, DeviceArray):
        _lib.synchronize(dev)      # (a foreign input may be freed by its owner as soon as we return)
    return out


class DepthGate:
    """The gate of the depth-consistency weights (include/smesh_depth.h, where the rule is stated to the bit): a pixel keeps its
    weight when |rendered depth - sensor depth| <= abs_tol + rel_tol * sensor depth, in float32, the sensor depth being
    raw * `scale`.  `abs_tol` has no default: the caller states it.  `scale` None: 0.001 for integer sensor images (ScanNet's
    millimetres), 1.0 for float ones.  `max_depth`: rendered depths beyond it get weight 0 (None: no limit).  `missing`: what a
    pixel without a measurement (raw 0; a float sample that is not a positive finite number) gets -- "keep" its weight (no
    evidence against it, the ungated behaviour) or "drop" it."""

    def __init__(self, abs_tol, rel_tol=0.0, scale=None, max_depth=None, missing="keep"):
        def number(v, name, allow_inf=False):
            try:
                f = float(np.float32(v))
            except (TypeError, ValueError):
                raise ValueError("DepthGate: %s must be a number, got %r" % (name, v))
            if f != f or f < 0.0 or (not allow_inf and f == float("inf")):
                raise ValueError("DepthGate: %s must be a finite number >= 0, got %r" % (name, v))
            return f
        self.abs_tol = number(abs_tol, "abs_tol")
        self.rel_tol = number(rel_tol, "rel_tol")
        self.scale = None if scale is None else number(scale, "scale")
        if max_depth is None:
            self.max_depth = None
        else:
            try:
                self.max_depth = float(np.float32(max_depth))
            except (TypeError, ValueError):
                raise ValueError("DepthGate: max_depth must be a number or None, got %r" % (max_depth,))
            if self.max_depth != self.max_depth:
                raise ValueError("DepthGate: max_depth must not be NaN")
        if missing not in ("keep", "drop"):
            raise ValueError('DepthGate: missing must be "keep" or "drop", got %r' % (missing,))
        self.missing = missing

    def scale_for(self, dtype):
        """The scale applied to a sensor image of `dtype`."""
        if self.scale is not None:
            return self.scale
        return 0.001 if np.dtype(dtype).kind in "iu" else 1.0

    def _pod(self, dtype):
        return _lib.DepthGatePOD(self.scale_for(dtype), self.abs_tol, self.rel_tol,
                                 float("inf") if self.max_depth is None else self.max_depth, 1 if self.missing == "keep" else 0)

    def __repr__(self):
        return "DepthGate(abs_tol=%r, rel_tol=%r, scale=%r, max_depth=%r, missing=%r)" % (self.abs_tol, self.rel_tol, self.scale, self.max_depth, self.missing)


_DEPTH_CODES = {"uint16": _lib.DEPTH_U16, "float32": _lib.DEPTH_F32}


def _describe_sensor(sensor, device, streams, what="sensor depth image"):
    """(pointer, memkind, (w, h), dtype code, element strides, keep-alive, numpy dtype) of a sensor depth image: (w,h) uint16 or
    float32, host numpy or device array, any non-negative strides -- a decoded (h,w) image goes over as its transposed view."""
    sp, smem, sshape, sdt, sstr, keep = describe(sensor, 2, what, device, streams)
    if sdt.name not in _DEPTH_CODES:
        raise ValueError("%s dtype must be uint16 or float32, got %s" % (what, sdt))
    if not (sshape[0] and sshape[1]):
        raise ValueError("an empty %s %s cannot be sampled" % (what, tuple(sshape)))
    return sp, smem, (int(sshape[0]), int(sshape[1])), _DEPTH_CODES[sdt.name], tuple(sstr), keep, sdt


def _dense_plane(image, W, H, device, what, streams, dtype=np.float32):
    """`image` as a dense (W,H) plane of `dtype` (float32; uint32 for an index plane) in device memory (a host array is copied
    there): (pointer, keep-alive)."""
    from .device import to_device
    dtype = np.dtype(dtype)
    ptr, mem, shape, dt, strides, keep = describe(image, 2, what, device, streams)
    if mem == _lib.MEM_HOST:
        if not isinstance(keep, np.ndarray) or (dt.kind != "f" if dtype.kind == "f" else dt != dtype):
            raise ValueError("%s must be a %s array, got %s" % (what, dtype, dt))
        keep = to_device(np.ascontiguousarray(keep, dtype=dtype), device)
        ptr, shape, dt, strides = keep.ptr, keep.shape, keep.dtype, keep.strides
    if tuple(shape) != (W, H) or dt != dtype or tuple(strides) != (H, 1):
        raise ValueError("%s must be contiguous %s (W,H) = %s, got %s %s" % (what, dtype, (W, H), dt, tuple(shape)))
    return ptr, keep


def depth_weights_device(depth, sensor_depth, gate, weights_image=None, device=0, return_counts=False):
    """The depth-consistency weights of ONE view on the device (`smesh_depth_weights`, include/smesh_depth.h): `depth` the float32
    (W,H) depth plane of `renderer.render(camera)` (or a host copy of one), `sensor_depth` the sensor's (w,h) uint16 / float32 image
    (host numpy or device array, any non-negative strides; sampled nearest with half-pixel centres where its size differs),
    `gate` a `DepthGate`, `weights_image` an optional float32 (W,H) image that is multiplied in.  Returns a float32 (W,H)
    `DeviceArray` -- what `add(idx, probs, w)` takes as its weights image; with `return_counts=True` also the uint64
    [visible, far, missing, inconsistent] counts, which makes the call wait."""
    from .device import DeviceBuffer
    if not isinstance(gate, DepthGate):
        raise ValueError("depth_gate must be a fusion.DepthGate, got %r" % (gate,))
    if isinstance(depth, DeviceArray):
        device = depth.device
    device = int(device)
    shape = tuple(getattr(depth, "shape", None) or np.shape(depth))
    if len(shape) != 2:
        raise ValueError("depth plane must have rank 2, got shape %s" % (shape,))
    W, H = int(shape[0]), int(shape[1])
    streams = []
    sp, smem, (w, h), scode, sstr, skeep, sdt = _describe_sensor(sensor_depth, device, streams)
    dp, dkeep = _dense_plane(depth, W, H, device, "depth plane", streams)
    wp, wkeep = (None, None) if weights_image is None else _dense_plane(weights_image, W, H, device, "weights image", streams)
    out = DeviceBuffer(max(W * H * 4, 4), device).view((W, H), np.float32)
    counts = np.zeros(4, np.uint64) if return_counts else None
    pod = gate._pod(sdt)
    _lib.check(_lib.lib().smesh_depth_weights(ctypes.c_void_p(dp), W, H, ctypes.c_void_p(sp), scode, _c64(sstr), smem, w, h, ctypes.byref(pod),
                                              None if wp is None else ctypes.c_void_p(wp), ctypes.c_void_p(out.ptr),
                                              None if counts is None else counts.ctypes.data_as(ctypes.c_void_p), device))
    release_to(device, streams)
    if any(k is not None and not isinstance(k, (DeviceArray, np.ndarray)) for k in (skeep, dkeep, wkeep)):
        _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)
    out._gate_inputs = (dkeep, wkeep, skeep)      # (this library's own arrays are freed behind its streams)
    return (out, counts) if return_counts else out


def depth_weights(depth, sensor_depth, gate, weights_image=None, device=0, return_counts=False):
    """`depth_weights_device` copied to the host: a numpy array (and the counts)."""
    r = depth_weights_device(depth, sensor_depth, gate, weights_image, device, return_counts)
    return (r[0].numpy(), r[1]) if return_counts else r.numpy()


def _gate_keywords(sensor_depths, depth_gate, depth_stats, n, sample_in_kernel, what):
    """The `sensor_depth(s)=`, `depth_gate=` and `depth_stats=` keywords of a fuse call of `n` views, checked: None for a call
    without them, else the list of sensor images."""
    if sensor_depths is None and depth_gate is None:
        if depth_stats:
            raise ValueError("%s: depth_stats=True needs sensor depths and a depth_gate" % what)
        return None
    if sensor_depths is None or depth_gate is None:
        raise ValueError("%s: sensor depths and depth_gate go together, one was given without the other" % what)
    if not isinstance(depth_gate, DepthGate):
        raise ValueError("%s: depth_gate must be a fusion.DepthGate, got %r" % (what, depth_gate))
    if sample_in_kernel:
        raise ValueError("%s: sample_in_kernel=True cannot be combined with a depth gate" % what)
    sensors = list(sensor_depths)
    if len(sensors) != n:
        raise ValueError("%s needs one sensor depth image per camera: %d for %d cameras" % (what, len(sensors), n))
    return sensors


class ViewWeights:
    """The spec of the viewing-geometry weights (include/smesh_view_weights.h, where the rule is stated to the bit): a pixel's weight
    is cos^`power` of the angle between its ray and the normal of the face it shows (an integer power, 0 .. 16), times
    1 / (1 + (depth / `falloff_depth`)^2) where a falloff is given.  `min_cos`: pixels seen at a smaller cosine get weight 0.
    `two_sided=False`: faces that look away from the camera get weight 0.  `max_depth`: rendered depths beyond it get weight 0
    (None: no limit).  Triangle renderers only."""

    def __init__(self, power=1, min_cos=0.0, two_sided=True, max_depth=None, falloff_depth=None):
        if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 0 <= int(power) <= _lib.VW_MAX_POWER:
            raise ValueError("ViewWeights: power must be an integer in [0, %d], got %r" % (_lib.VW_MAX_POWER, power))
        self.power = int(power)

        def number(v, name):
            try:
                f = float(np.float32(v))
            except (TypeError, ValueError):
                raise ValueError("ViewWeights: %s must be a number, got %r" % (name, v))
            if f != f:
                raise ValueError("ViewWeights: %s must not be NaN" % name)
            return f
        self.min_cos = number(min_cos, "min_cos")
        if not 0.0 <= self.min_cos <= 1.0:
            raise ValueError("ViewWeights: min_cos must be in [0, 1], got %r" % (min_cos,))
        if not isinstance(two_sided, (bool, np.bool_)):
            raise ValueError("ViewWeights: two_sided must be True or False, got %r" % (two_sided,))
        self.two_sided = bool(two_sided)
        self.max_depth = None if max_depth is None else number(max_depth, "max_depth")
        self.falloff_depth = None if falloff_depth is None else number(falloff_depth, "falloff_depth")
        if self.falloff_depth is not None and not self.falloff_depth > 0.0:
            raise ValueError("ViewWeights: falloff_depth must be > 0 or None, got %r" % (falloff_depth,))

    def _pod(self):
        inf = float("inf")
        return _lib.ViewWeightsPOD(self.power, self.min_cos, 1 if self.two_sided else 0, inf if self.max_depth is None else self.max_depth,
                                   inf if self.falloff_depth is None else self.falloff_depth)

    def __repr__(self):
        return "ViewWeights(power=%r, min_cos=%r, two_sided=%r, max_depth=%r, falloff_depth=%r)" % (
            self.power, self.min_cos, self.two_sided, self.max_depth, self.falloff_depth)


def _triangle_renderer(renderer, what):
    if getattr(renderer, "is_texel", False):
        raise ValueError("%s: view weights need a triangle renderer -- the index plane of a texel renderer holds texel ids, and a "
                         "texel -> face lookup is not built" % what)


def view_weights_device(renderer, camera, primitive_indices, depth, spec, weights_image=None, return_counts=False):
    """The viewing-geometry weights of ONE view on the device (`smesh_view_weights`, include/smesh_view_weights.h):
    `primitive_indices`, `depth` the uint32 and float32 (W,H) planes of `renderer.render(camera)` (or host copies of them), `spec` a
    `ViewWeights`, `weights_image` an optional float32 (W,H) image that is multiplied in.  Returns a float32 (W,H) `DeviceArray` --
    what `add(idx, probs, w)`, `add_many`, `add_labels` and `fuse_views_ranged` take as a weights image; with `return_counts=True`
    also the uint64 [visible, far, grazing, backfacing] counts, which makes the call wait."""
    from .device import DeviceBuffer
    if not isinstance(spec, ViewWeights):
        raise ValueError("view_weights must be a fusion.ViewWeights, got %r" % (spec,))
    _triangle_renderer(renderer, "view_weights")
    device = int(renderer.device)
    W, H = camera.resolution
    W, H = int(W), int(H)
    streams = []
    ip, ikeep = _dense_plane(primitive_indices, W, H, device, "primitive index plane", streams, np.uint32)
    dp, dkeep = _dense_plane(depth, W, H, device, "depth plane", streams)
    wp, wkeep = (None, None) if weights_image is None else _dense_plane(weights_image, W, H, device, "weights image", streams)
    out = DeviceBuffer(max(W * H * 4, 4), device).view((W, H), np.float32)
    counts = np.zeros(4, np.uint64) if return_counts else None
    pod = spec._pod()
    _lib.check(_lib.lib().smesh_view_weights(renderer._h, ctypes.byref(camera._pod), ctypes.c_void_p(ip), ctypes.c_void_p(dp), W, H, ctypes.byref(pod),
                                             None if wp is None else ctypes.c_void_p(wp), ctypes.c_void_p(out.ptr),
                                             None if counts is None else counts.ctypes.data_as(ctypes.c_void_p)))
    release_to(device, streams)
    if any(k is not None and not isinstance(k, (DeviceArray, np.ndarray)) for k in (ikeep, dkeep, wkeep)):
        _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)
    out._gate_inputs = (ikeep, dkeep, wkeep)      # (this library's own arrays are freed behind its streams)
    return (out, counts) if return_counts else out


def view_weights(renderer, camera, primitive_indices, depth, spec, weights_image=None, return_counts=False):
    """`view_weights_device` copied to the host: a numpy array (and the counts)."""
    r = view_weights_device(renderer, camera, primitive_indices, depth, spec, weights_image, return_counts)
    return (r[0].numpy(), r[1]) if return_counts else r.numpy()


def _view_keywords(renderer, view_weights, view_stats, sample_in_kernel, what):
    """The `view_weights=` and `view_stats=` keywords of a fuse call, checked: None for a call without them, else the spec."""
    if view_weights is None:
        if view_stats:
            raise ValueError("%s: view_stats=True needs view_weights" % what)
        return None
    if not isinstance(view_weights, ViewWeights):
        raise ValueError("%s: view_weights must be a fusion.ViewWeights, got %r" % (what, view_weights))
    if sample_in_kernel:
        raise ValueError("%s: sample_in_kernel=True cannot be combined with view weights" % what)
    _triangle_renderer(renderer, what)
    return view_weights


def _stats_of(view_counts, depth_counts, view_stats, depth_stats, single=False, edge_counts=None, edge_stats=False):
    """What a weighted / gated fuse call returns: None, one uint64 counts array bare, or the tuple of those asked for in the order
    (view counts, edge counts, depth counts)."""
    got = [c[0] if single else c for c, asked in ((view_counts, view_stats), (edge_counts, edge_stats), (depth_counts, depth_stats)) if asked]
    return None if not got else got[0] if len(got) == 1 else tuple(got)


class EdgeGate:
    """The gate of the occlusion-edge weights (include/smesh_edge_gate.h, where the rule is stated to the bit): a pixel of the rendered
    depth plane loses its weight when a depth discontinuity lies within `radius` pixels (1 .. 8, a square window) of it.  With d the
    pixel's depth, lo / hi the smallest / largest finite depth in the window and t = abs_tol + rel_tol * d in float32: `behind` drops
    the pixel when d - lo > t (a nearer surface close by: its labels bleed onto this pixel), `front` when hi - d > t (the rim of an
    occluder), `silhouette` when the window holds background.  `abs_tol` has no default: the caller states it."""

    def __init__(self, radius, abs_tol, rel_tol=0.0, behind=True, front=False, silhouette=False):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= _lib.EDGE_MAX_RADIUS:
            raise ValueError("EdgeGate: radius must be an integer in [1, %d], got %r" % (_lib.EDGE_MAX_RADIUS, radius))
        self.radius = int(radius)

        def number(v, name):
            try:
                f = float(np.float32(v))
            except (TypeError, ValueError):
                raise ValueError("EdgeGate: %s must be a number, got %r" % (name, v))
            if f != f or f < 0.0 or f == float("inf"):
                raise ValueError("EdgeGate: %s must be a finite number >= 0, got %r" % (name, v))
            return f
        self.abs_tol = number(abs_tol, "abs_tol")
        self.rel_tol = number(rel_tol, "rel_tol")
        for name, v in (("behind", behind), ("front", front), ("silhouette", silhouette)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("EdgeGate: %s must be True or False, got %r" % (name, v))
        self.behind, self.front, self.silhouette = bool(behind), bool(front), bool(silhouette)

    def _pod(self):
        return _lib.EdgeGatePOD(self.radius, self.abs_tol, self.rel_tol, int(self.behind), int(self.front), int(self.silhouette))

    def __repr__(self):
        return "EdgeGate(radius=%r, abs_tol=%r, rel_tol=%r, behind=%r, front=%r, silhouette=%r)" % (
            self.radius, self.abs_tol, self.rel_tol, self.behind, self.front, self.silhouette)


def edge_weights_device(depth, gate, weights_image=None, return_counts=False, device=0):
    """The occlusion-edge weights of ONE view on the device (`smesh_edge_weights`, include/smesh_edge_gate.h): `depth` the float32
    (W,H) depth plane of `renderer.render(camera)` (a host copy of one, or any plane of the caller's), `gate` an `EdgeGate`,
    `weights_image` an optional float32 (W,H) image that is multiplied in.  Returns a float32 (W,H) `DeviceArray` -- what
    `add(idx, probs, w)`, `add_many`, `add_labels` and `fuse_views_ranged` take as a weights image; with `return_counts=True` also the
    uint64 [visible, behind, front, silhouette] counts, which makes the call wait.  A host plane goes to `device`."""
    from .device import DeviceBuffer
    if not isinstance(gate, EdgeGate):
        raise ValueError("edge_gate must be a fusion.EdgeGate, got %r" % (gate,))
    if isinstance(depth, DeviceArray):
        device = depth.device
    device = int(device)
    shape = tuple(getattr(depth, "shape", None) or np.shape(depth))
    if len(shape) != 2:
        raise ValueError("depth plane must have rank 2, got shape %s" % (shape,))
    W, H = int(shape[0]), int(shape[1])
    streams = []
    dp, dkeep = _dense_plane(depth, W, H, device, "depth plane", streams)
    wp, wkeep = (None, None) if weights_image is None else _dense_plane(weights_image, W, H, device, "weights image", streams)
    out = DeviceBuffer(max(W * H * 4, 4), device).view((W, H), np.float32)
    counts = np.zeros(4, np.uint64) if return_counts else None
    pod = gate._pod()
    _lib.check(_lib.lib().smesh_edge_weights(ctypes.c_void_p(dp), W, H, ctypes.byref(pod), None if wp is None else ctypes.c_void_p(wp),
                                             ctypes.c_void_p(out.ptr), None if counts is None else counts.ctypes.data_as(ctypes.c_void_p), device))
    release_to(device, streams)
    if any(k is not None and not isinstance(k, (DeviceArray, np.ndarray)) for k in (dkeep, wkeep)):
        _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)
    out._gate_inputs = (dkeep, wkeep)      # (this library's own arrays are freed behind its streams)
    return (out, counts) if return_counts else out


def edge_weights(depth, gate, weights_image=None, return_counts=False, device=0):
    """`edge_weights_device` copied to the host: a numpy array (and the counts)."""
    r = edge_weights_device(depth, gate, weights_image, return_counts, device)
    return (r[0].numpy(), r[1]) if return_counts else r.numpy()


def _edge_keywords(edge_gate, edge_stats, sample_in_kernel, what):
    """The `edge_gate=` and `edge_stats=` keywords of a fuse call, checked: None for a call without them, else the gate."""
    if edge_gate is None:
        if edge_stats:
            raise ValueError("%s: edge_stats=True needs edge_gate" % what)
        return None
    if not isinstance(edge_gate, EdgeGate):
        raise ValueError("%s: edge_gate must be a fusion.EdgeGate, got %r" % (what, edge_gate))
    if sample_in_kernel:
        raise ValueError("%s: sample_in_kernel=True cannot be combined with an edge gate" % what)
    return edge_gate


GROUP_VIEWS = 8                                                     # views per deferred group (= the library's views per launch)
DEFER_VIEWS = os.environ.get("SMESH_DEFER_VIEWS", "1") != "0"       # default of MeshAggregator.defer

import weakref                                                       # noqa: E402
_aggregators = weakref.WeakSet()
_aggregators_lock = threading.Lock()      # (aggregators are created and flushed from different threads in the harness)


def _flush_device(device=None):
    with _aggregators_lock:
        live = list(_aggregators)
    for a in live:
        if (device is None or a.device == device) and a._pending:
            a.flush()


_lib._flush_hooks.append(_flush_device)


class _PodCamera:
    """The camera of a render() plane that has not been rasterised yet, as `_fuse_views_sampled` reads cameras."""

    def __init__(self, pod, W, H):
        self._pod, self.resolution = pod, (W, H)


class _MeshAggregator:
    def __init__(self, primitives, classes, kind, images_equal_weight, device):
        self.primitives, self.classes = int(primitives), int(classes)
        self.kind, self.images_equal_weight, self.device = kind, float(images_equal_weight), int(device)
        if self.primitives < 0 or self.classes <= 0:
            raise ValueError("primitives must be >= 0 and classes > 0")
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_aggregator_create(self.primitives, self.classes, _lib.AGG_KINDS[kind],
                                                     self.images_equal_weight, self.device, ctypes.byref(h)))
        self._handle = h
        self._inflight = []     # (completion token, [objects]) of asynchronous calls whose device inputs may still be being read
        self._inflight_lock = threading.Lock()   # (the harness adds from a worker thread while the main thread may call get())
        # Deferred views (round 6): add() of a not-yet-rasterised render() plane and fuse_view(), with class vectors in this library's own
        # device arrays, are taken into a group of up to eight views that go to the library as ONE smesh_fuse_views call -- the views
        # share their rasteriser launches and each accumulator row makes one round trip for all of them: the batch entry point's
        # throughput behind the reference's per-view loop (colorize_cityscapes_mesh.py:54-67).  Same sums in the same order.  The group
        # is handed over on the eighth view, at anything else that uses the aggregator (`_h`), at `flush()`, at `_lib.synchronize()`.
        self._pending = []      # [(renderer, CameraPOD, W, H, probs array -- or label plane --, weights array or None, is a label view, SMESH_PROBS_* of a probs array)]
        self._pending_lock = threading.RLock()
        self.defer = DEFER_VIEWS
        with _aggregators_lock:
            _aggregators.add(self)

    @property
    def _h(self):
        """The library handle -- for a call that is about to use it: every deferred view is handed over first."""
        if self._pending:
            self.flush()
        return self._handle

    def flush(self):
        """Hand the deferred views (see __init__) to the library now.  Asynchronous like fuse_views: nothing is waited for."""
        with self._pending_lock:
            todo, self._pending = self._pending, []
            if not todo:
                return
            renderer = todo[0][0]
            n = len(todo)
            pods = (_lib.CameraPOD * n)(*[t[1] for t in todo])
            pptr = (ctypes.c_void_p * n)(*[t[4].ptr for t in todo])
            wptr = None
            if todo[0][5] is not None:
                wptr = (ctypes.c_void_p * n)(*[t[5].ptr for t in todo])
            if todo[0][6]:     # a group of label views (all-labels or all-probs, one label dtype: _defer)
                _lib.check(_lib.lib().smesh_fuse_views_labels(renderer._h, self._handle, pods, n, pptr, _lib.LBL_CODES[todo[0][4].dtype.name],
                                                              None, wptr, _lib.MEM_DEVICE))
                return
            if todo[0][7] != _lib.PROBS_F32:     # a group of float16 / bfloat16 images (one dtype: _defer)
                _lib.check(_lib.lib().smesh_fuse_views_probs16(renderer._h, self._handle, pods, n, pptr, todo[0][7], wptr, _lib.MEM_DEVICE))
                return
            _lib.check(_lib.lib().smesh_fuse_views(renderer._h, self._handle, pods, n, pptr, wptr, _lib.MEM_DEVICE))
            # (the class vectors are this library's own arrays: freed behind its streams, no completion token needed)

    def _deferrable(self, probs_image, weights_image, W, H, probs_dtype=None):
        """May a view with these inputs wait for its group?  Only with inputs nobody else can write to behind our back: this library's
        own dense float32 / float16 / bfloat16 device arrays that were never exported to another framework (anything else is consumed
        by the call itself, in order: foreign device tensors may be re-used by their owner as soon as the call returns, host arrays
        likewise).  Returns None, or the SMESH_PROBS_* code of the class vectors (0 is float32: test with `is not None`)."""
        if not self.defer:
            return None
        if type(probs_image) is not DeviceArray:
            return None
        try:
            code = probs_code(probs_image.dtype, probs_image, probs_dtype)
        except ValueError:
            return None       # (the call itself raises it)
        ok = (code is not None and not probs_image._exported and probs_image.device == self.device
              and probs_image.shape == (W, H, self.classes)
              and probs_image.strides == (H * self.classes, self.classes, 1))
        if ok and weights_image is not None:
            ok = (type(weights_image) is DeviceArray and not weights_image._exported and weights_image.device == self.device
                  and weights_image.dtype == np.float32 and weights_image.shape == (W, H) and weights_image.strides == (H, 1))
        return code if ok else None

    def _deferrable_labels(self, label_image, weights_image, W, H):
        """`_deferrable` for a label view: this library's own dense uint8 / uint16 device plane, never exported."""
        if not self.defer:
            return False
        ok = (type(label_image) is DeviceArray and not label_image._exported and label_image.device == self.device
              and label_image.dtype in (np.uint8, np.uint16) and label_image.shape == (W, H) and label_image.strides == (H, 1))
        if ok and weights_image is not None:
            ok = (type(weights_image) is DeviceArray and not weights_image._exported and weights_image.device == self.device
                  and weights_image.dtype == np.float32 and weights_image.shape == (W, H) and weights_image.strides == (H, 1))
        return ok

    def _defer(self, renderer, pod, W, H, probs_image, weights_image, labels=False, code=_lib.PROBS_F32):
        with self._pending_lock:
            if self._pending:
                first = self._pending[0]
                # one group = one renderer, one image size, weights for all views or for none, class vectors (of one dtype) or labels
                # (of one dtype)
                if (first[0] is not renderer or (first[2], first[3]) != (W, H) or (first[5] is None) != (weights_image is None)
                        or first[6] != labels or first[7] != code or (labels and first[4].dtype != probs_image.dtype)):
                    self.flush()
            self._pending.append((renderer, pod, W, H, probs_image, weights_image, labels, code))
            if len(self._pending) >= GROUP_VIEWS:
                self.flush()

    def _hold(self, keepalives):
        """The asynchronous entry points read DEVICE images after they return.  `release_to()` orders the stream `describe()` guessed for
        their owner behind those reads -- but a tensor that is later freed or re-used on ANOTHER stream or thread (or whose producer
        exported no stream) could be recycled by its caching allocator while the kernels still read it.  So the aggregator keeps its own
        references to the inputs of other frameworks until a completion token recorded behind the call is done (checked, without waiting,
        at the next call).  This library's own DeviceArrays are freed behind its streams and need none."""
        self._drain()
        foreign = [k for k in keepalives if k is not None and not isinstance(k, DeviceArray)]
        if not foreign:
            return
        tok = ctypes.c_uint64(0)
        _lib.check(_lib.lib().smesh_token_record(self.device, ctypes.byref(tok)))
        with self._inflight_lock:
            self._inflight.append((tok.value, foreign))

    def _drain(self):
        done = ctypes.c_int(0)
        with self._inflight_lock:      # (a token goes back to the library's pool exactly once)
            while self._inflight:
                _lib.check(_lib.lib().smesh_token_done(self.device, ctypes.c_uint64(self._inflight[0][0]), ctypes.byref(done)))
                if not done.value:
                    break
                self._inflight.pop(0)

    def _resampled(self, probs_image, size, mode, probs_dtype):
        """`probs_image` as a view of `size` = (W,H) takes it (the `resize=` keyword of add / add_many / fuse_view / fuse_views,
        include/smesh_resize.h): itself where `mode` is None or its width and height are the view's already; else its resampled
        image -- a dense DeviceArray of the input's dtype that this library owns and nobody else has seen, which is what `_deferrable`
        asks for, so such views still gather in groups of eight and 16-bit images still reach the 16-bit kernel.  The kernel runs on
        the library's main stream, ahead of the fusion that reads its output.  (An image that does not say its shape -- a DLPack
        capsule -- is resampled whatever its size: equal sizes give an exact copy.)"""
        if mode is None:
            return probs_image
        from .resize import _resize_device, image_size
        if image_size(probs_image) == tuple(size):
            return probs_image
        return _resize_device(probs_image, tuple(size), None, probs_dtype, mode, self.device, hold=self._hold)

    # ---- sample_in_kernel=True (include/smesh_sampled.h): the small image goes to the library as it is ----------------------------
    @staticmethod
    def _sampling_mode(resize, sample_in_kernel, what):
        """The SMESH_RESIZE_* code of a call with `sample_in_kernel=True`, None for a call without it."""
        from .resize import resize_mode
        mode = resize_mode(resize)
        if not sample_in_kernel:
            return None
        if mode is None:
            raise ValueError('%s: sample_in_kernel=True is only meaningful together with resize="bilinear"' % what)
        return mode

    def _describe_sampled(self, probs_image, probs_dtype, streams, what="probs image"):
        """`_describe_probs` of a (w,h,C) image for the sampled entry points: the class count is the aggregator's."""
        from .evaluation import _describe_probs
        d = _describe_probs(probs_image, probs_dtype, self.device, streams, what)
        if d[2][2] != self.classes:
            raise ValueError("%s has %d classes, aggregator was built for %d" % (what, d[2][2], self.classes))
        if d[2][0] < 1 or d[2][1] < 1:
            raise ValueError("an empty %s %s cannot be resampled" % (what, d[2][:2]))
        return d

    def _fuse_views_sampled(self, renderer, cameras, probs_images, weights_images, probs_dtype, mode, what):
        """`fuse_views(..., resize="bilinear", sample_in_kernel=True)`: every image is checked first, then consecutive images of one
        size, layout, dtype and memory go to `smesh_fuse_views_sampled` as one batch -- the library groups them by eight."""
        cameras, probs_images = list(cameras), list(probs_images)
        wts = None if weights_images is None else list(weights_images)
        n = len(cameras)
        if len(probs_images) != n or (wts is not None and len(wts) != n):
            raise ValueError("%s needs one probs image (and one weights image or None) per camera" % what)
        streams, desc = [], []
        for i, cam in enumerate(cameras):
            W, H = cam.resolution
            d = self._describe_sampled(probs_images[i], probs_dtype, streams, "probs image %d" % i)
            dw = None
            if wts is not None and wts[i] is not None:
                dw = self._describe_weights(wts[i], streams)
                if dw[2] != (W, H) or dw[3] != (H, 1) or dw[1] != d[1]:
                    raise ValueError("weights image %d must be contiguous float32 (W,H) in the same memory as probs" % i)
            elif wts is not None:
                raise ValueError("%s: weights for every view or for none" % what)
            desc.append((d, dw))
        lo = 0
        while lo < n:
            first = desc[lo][0]
            hi = lo + 1
            while hi < n and desc[hi][0][1:5] == first[1:5]:
                hi += 1
            m = hi - lo
            pods = (_lib.CameraPOD * m)(*[cam._pod for cam in cameras[lo:hi]])
            pptr = (ctypes.c_void_p * m)(*[d[0] for d, _ in desc[lo:hi]])
            wptr = None if wts is None else (ctypes.c_void_p * m)(*[dw[0] for _, dw in desc[lo:hi]])
            _lib.check(_lib.lib().smesh_fuse_views_sampled(renderer._h, self._h, pods, m, pptr, first[3], _c64(first[4]), first[2][0], first[2][1],
                                                           wptr, first[1], mode))
            lo = hi
        release_to(self.device, streams)
        self._hold([d[5] for d, _ in desc if d[1] == _lib.MEM_DEVICE] + [dw[4] for d, dw in desc if dw is not None and d[1] == _lib.MEM_DEVICE])

    def _add_sampled(self, primitive_image, probs_image, weights_image, probs_dtype, mode):
        """`add(..., resize="bilinear", sample_in_kernel=True)`: the views already deferred are handed over first (the order of
        additions stays the caller's), then this view is one library call -- a render() plane that has not been rasterised yet is
        never produced (`smesh_fuse_view_sampled` with its camera), any other index image goes to `smesh_aggregator_add_sampled`."""
        streams = []
        pp, pmem, (w, h, C), code, pstr, k1 = self._describe_sampled(probs_image, probs_dtype, streams)
        wdesc = None if weights_image is None else self._describe_weights(weights_image, streams)
        ishape = tuple(getattr(primitive_image, "shape", None) or np.shape(primitive_image))
        if len(ishape) != 2 or (wdesc is not None and wdesc[2] != ishape):
            raise ValueError("Primitive image %s and weights image %s must have the same width and height"
                             % (ishape, None if wdesc is None else wdesc[2]))
        lazy = getattr(primitive_image, "unrun", False) and primitive_image._which == 0 and primitive_image.device == self.device
        if lazy and (wdesc is None or (wdesc[3] == (ishape[1], 1) and wdesc[1] == pmem)):
            pend = primitive_image._pending
            if pend.W and pend.H:      # (an empty plane adds nothing and hands nothing over, like every other empty-image return)
                self.flush()
                _lib.check(_lib.lib().smesh_fuse_view_sampled(pend.renderer._h, self._handle, ctypes.byref(pend.pod), ctypes.c_void_p(pp), code,
                                                              _c64(pstr), w, h, None if wdesc is None else ctypes.c_void_p(wdesc[0]), pmem, mode))
                release_to(self.device, streams)
                self._hold([k1 if pmem == _lib.MEM_DEVICE else None, wdesc[4] if (wdesc is not None and wdesc[1] == _lib.MEM_DEVICE) else None])
            return
        ip, imem, ishape, idt, istr, k0 = describe(primitive_image, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        W, H = ishape
        if W == 0 or H == 0:
            return
        rb = getattr(primitive_image, "_rendered_by", None)
        if not (rb is not None and not primitive_image._exported and getattr(rb, "_h", None) is not None and rb._h.value
                and rb.device == self.device):
            rb = None
        wp, wmem, wstr, k2 = (None, _lib.MEM_HOST, None, None) if wdesc is None else (wdesc[0], wdesc[1], wdesc[3], wdesc[4])
        _lib.check(_lib.lib().smesh_aggregator_add_sampled(
            self._h, None if rb is None else rb._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
            ctypes.c_void_p(pp), code, _c64(pstr), pmem,
            None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, w, h, W, H, mode))
        release_to(self.device, streams)
        self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if pmem == _lib.MEM_DEVICE else None,
                    k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])

    # ---- views gated by sensor depth (include/smesh_depth.h) ---------------------------------------------------------------------
    def _gated_probs(self, image, W, H, mode, probs_dtype, streams, what):
        """A class-vector image of a gated call as the library takes it: resampled where `resize=` asks for it, copied to the device
        where it is a host array -- (pointer, SMESH_PROBS_* code, keep-alive) of a dense (W,H,C) device image."""
        from .device import to_device
        image = self._resampled(image, (W, H), mode, probs_dtype)
        pp, pmem, pshape, pdt, pstr, k1 = describe(image, 3, what, self.device, streams)
        code = probs_code(pdt, k1, probs_dtype, what)
        if tuple(pshape) != (W, H, self.classes) or code is None:
            raise ValueError("%s must be float32, float16 or bfloat16 (W,H,C) = %s" % (what, (W, H, self.classes)))
        if pmem == _lib.MEM_HOST:
            if not isinstance(k1, np.ndarray):
                raise ValueError("%s: a host image of a gated fuse call must be a numpy array" % what)
            dev = to_device(np.ascontiguousarray(k1), self.device)
            dev.bfloat16 = code == _lib.PROBS_BF16
            return dev.ptr, code, dev
        if pstr != (H * self.classes, self.classes, 1):
            raise ValueError("a gated fuse call needs contiguous (W,H,C) probs images on the device")
        return pp, code, k1

    def _gated_labels(self, image, W, H, resize, m, streams, what):
        """A label image of a gated call as the library takes it: (pointer, SMESH_DEPTH_IMG_LABELS_* code, keep-alive) of a dense
        (W,H) uint8 / uint16 device plane -- this library's own dense plane as it is, anything else through `prepare_labels_device`
        (sampled, mapped, narrowed)."""
        if (m is None and type(image) is DeviceArray and image.device == self.device and image.shape == (W, H) and image.strides == (H, 1)
                and (image.dtype == np.uint16 or (image.dtype == np.uint8 and self.classes <= 255))):
            plane = image
        else:
            table = m if isinstance(m, ColorTable) else None
            plane = prepare_labels_device(image, self.classes, (W, H), resize, None if table is not None else m, self.device, table)
        return plane.ptr, (_lib.DEPTH_IMG_LABELS_U8 if plane.dtype == np.uint8 else _lib.DEPTH_IMG_LABELS_U16), plane

    def _fuse_views_gated(self, renderer, cameras, prepare, weights_images, sensors, gate, depth_stats, what, spec=None, view_stats=False,
                          edge=None, edge_stats=False):
        """The gated / weighted form of fuse_views / fuse_views_labels: the batch is worked through in chunks of eight views -- the views
        of a fusion launch; `prepare(i, streams)` gives view i's dense device image as (pointer, image kind, keep-alive), host weights are
        copied to the device, and a chunk whose sensor images share size, dtype, strides and memory (and whose images share their kind)
        is ONE `smesh_fuse_views_depth` call -- with `spec` (a `ViewWeights`) one `smesh_fuse_views_view_weights` call, with or without
        sensor images, with `edge` (an `EdgeGate`) one `smesh_fuse_views_weighted` call with whichever of the three stages are given;
        a mixed chunk goes view by view.  Returns (view counts or None, depth counts or None, edge counts or None), uint64 [n, 4] each."""
        n = len(cameras)
        counts = np.zeros((n, 4), np.uint64) if depth_stats else None
        vcounts = np.zeros((n, 4), np.uint64) if view_stats else None
        ecounts = np.zeros((n, 4), np.uint64) if edge_stats else None
        sensor_streams = []
        # (every sensor image is checked before anything is copied or fused)
        sdesc = None if sensors is None else [_describe_sensor(sensors[i], self.device, sensor_streams, "sensor depth image %d" % i) for i in range(n)]
        rh = renderer._h
        for lo in range(0, n, GROUP_VIEWS):
            hi = min(lo + GROUP_VIEWS, n)
            streams, views = [], []
            for i in range(lo, hi):
                W, H = cameras[i].resolution
                d_img = prepare(i, streams)
                d_s = None if sdesc is None else sdesc[i]
                wk = (None, None)
                if weights_images is not None and weights_images[i] is not None:
                    wk = _dense_plane(weights_images[i], W, H, self.device, "weights image %d" % i, streams)
                views.append((d_img, d_s, wk))
            runs, start = [], 0
            for j in range(1, len(views) + 1):
                if j == len(views) or views[j][0][1] != views[start][0][1] or (sdesc is not None and views[j][1][1:5] != views[start][1][1:5]):
                    runs.append((start, j))
                    start = j
            if len(runs) > 1:      # a mixed chunk: view by view
                runs = [(j, j + 1) for j in range(len(views))]
            for a, b in runs:
                k = b - a
                first_img, first_s = views[a][0], views[a][1]
                pods = (_lib.CameraPOD * k)(*[cameras[lo + j]._pod for j in range(a, b)])
                iptr = (ctypes.c_void_p * k)(*[views[j][0][0] for j in range(a, b)])
                sptr = None if sdesc is None else (ctypes.c_void_p * k)(*[views[j][1][0] for j in range(a, b)])
                wptr = None
                if any(views[j][2][0] is not None for j in range(a, b)):
                    wptr = (ctypes.c_void_p * k)(*[views[j][2][0] for j in range(a, b)])
                pod = None if sdesc is None else gate._pod(first_s[6])
                cptr = None if counts is None else ctypes.c_void_p(counts.ctypes.data + (lo + a) * 32)
                if edge is not None:
                    vpod, epod = None if spec is None else spec._pod(), edge._pod()
                    vptr = None if vcounts is None else ctypes.c_void_p(vcounts.ctypes.data + (lo + a) * 32)
                    eptr = None if ecounts is None else ctypes.c_void_p(ecounts.ctypes.data + (lo + a) * 32)
                    stail = (None, 0, None, 0, 0, 0, None) if sdesc is None else (sptr, first_s[3], _c64(first_s[4]), first_s[1], first_s[2][0],
                                                                                 first_s[2][1], ctypes.byref(pod))
                    _lib.check(_lib.lib().smesh_fuse_views_weighted(rh, self._h, pods, k, iptr, first_img[1], wptr,
                                                                    None if vpod is None else ctypes.byref(vpod), ctypes.byref(epod), *stail,
                                                                    vptr, eptr, cptr))
                    continue
                if spec is None:
                    _lib.check(_lib.lib().smesh_fuse_views_depth(rh, self._h, pods, k, iptr, first_img[1], wptr, sptr, first_s[3], _c64(first_s[4]),
                                                                 first_s[1], first_s[2][0], first_s[2][1], ctypes.byref(pod), cptr))
                    continue
                vpod = spec._pod()
                vptr = None if vcounts is None else ctypes.c_void_p(vcounts.ctypes.data + (lo + a) * 32)
                if sdesc is None:
                    _lib.check(_lib.lib().smesh_fuse_views_view_weights(rh, self._h, pods, k, iptr, first_img[1], wptr, ctypes.byref(vpod),
                                                                        None, 0, None, 0, 0, 0, None, vptr, None))
                else:
                    _lib.check(_lib.lib().smesh_fuse_views_view_weights(rh, self._h, pods, k, iptr, first_img[1], wptr, ctypes.byref(vpod),
                                                                        sptr, first_s[3], _c64(first_s[4]), first_s[1], first_s[2][0], first_s[2][1],
                                                                        ctypes.byref(pod), vptr, cptr))
            release_to(self.device, streams)
            self._hold([v[0][2] for v in views] + [v[1][5] for v in views if v[1] is not None and v[1][1] == _lib.MEM_DEVICE] + [v[2][1] for v in views])
        release_to(self.device, sensor_streams)
        return vcounts, counts, ecounts

    def _fuse_views_probs_gated(self, renderer, cameras, probs_images, weights_images, probs_dtype, resize, sensors, gate, depth_stats, what,
                                spec=None, view_stats=False, edge=None, edge_stats=False):
        from .resize import resize_mode
        mode = resize_mode(resize)
        cameras, probs_images = list(cameras), list(probs_images)
        wts = None if weights_images is None else list(weights_images)
        if len(probs_images) != len(cameras) or (wts is not None and len(wts) != len(cameras)):
            raise ValueError("%s needs one probs image (and one weights image or None) per camera" % what)

        def prepare(i, streams):
            W, H = cameras[i].resolution
            return self._gated_probs(probs_images[i], W, H, mode, probs_dtype, streams, "probs image %d" % i)
        return self._fuse_views_gated(renderer, cameras, prepare, wts, sensors, gate, depth_stats, what, spec, view_stats, edge, edge_stats)

    def _fuse_views_labels_gated(self, renderer, cameras, label_images, weights_images, resize, label_map, palette, sensors, gate, depth_stats, what,
                                 spec=None, view_stats=False, edge=None, edge_stats=False):
        label_resize_mode(resize)
        cameras, label_images = list(cameras), list(label_images)
        wts = None if weights_images is None else list(weights_images)
        if len(label_images) != len(cameras) or (wts is not None and len(wts) != len(cameras)):
            raise ValueError("%s needs one label image (and one weights image or None) per camera" % what)
        m = _palette_or_map(palette, label_map, label_images, self.classes, self.device) if cameras else None

        def prepare(i, streams):
            W, H = cameras[i].resolution
            return self._gated_labels(label_images[i], W, H, resize, m, streams, "label image %d" % i)
        return self._fuse_views_gated(renderer, cameras, prepare, wts, sensors, gate, depth_stats, what, spec, view_stats, edge, edge_stats)

    # ---- undistort=True (include/smesh_lens.h, lens.py): images on the sensor grid of a data.LensCamera ---------------------------
    def _fuse_views_undistorted(self, what, labels, renderer, cameras, images, weights_images, probs_dtype, resize, sample_in_kernel,
                                label_map, palette, sensor_depths, single, **gates):
        """The `undistort=True` form of fuse_view(s) / fuse_view(s)_labels: the batch is worked through in chunks of eight views -- the
        views of a fusion launch, so at most eight undistorted images are alive at once.  Every image handed over for a
        `data.LensCamera` is on that lens's sensor grid, at any size: a class-vector image becomes its undistorted (W,H,C) plane
        and its validity weights plane (the caller's (W,H) weights multiplied in), a mask its nearest-sampled plane with the
        don't-care code outside (a mask with `label_map=` / `palette=` is first turned into classes at its own size: the map is per
        pixel, so the order does not matter), a sensor depth image its nearest-sampled plane with 0, "missing", outside.  Each run
        of consecutive lens views, and each run of views that need nothing (a plain `Camera`; a lens without distortion seen
        through its default view at the image's size), then goes through the call without the keyword: the same additions as
        fusing those planes by hand, in the same order."""
        from .device import to_device
        from .lens import _undistort_pixels, _undistort_probs, is_plain
        from .resize import image_size
        if resize is not None or sample_in_kernel:
            raise ValueError("%s: undistort=True cannot be combined with resize= or sample_in_kernel=True (the sensor image is "
                             "undistorted at any size)" % what)
        cameras, images = list(cameras), list(images)
        n = len(cameras)
        wts = None if weights_images is None else list(weights_images)
        sensors = None if sensor_depths is None else list(sensor_depths)
        if len(images) != n or (wts is not None and len(wts) != n) or (sensors is not None and len(sensors) != n):
            raise ValueError("%s needs one image (and one weights image or None, one sensor depth image) per camera" % what)
        m = _palette_or_map(palette, label_map, images, self.classes, self.device) if (labels and n) else None
        table = m if isinstance(m, ColorTable) else None
        lmap = None if table is not None else m
        size_of = self._shape_of if labels else image_size
        plain = [is_plain(cam, size_of(img)) for cam, img in zip(cameras, images)]

        def call(lo, hi, imgs, w, s, through):
            if labels:
                return self.fuse_views_labels(renderer, cameras[lo:hi], imgs, w, label_map=lmap if through else None,
                                              palette=table if through else None, sensor_depths=s, **gates)
            return self.fuse_views(renderer, cameras[lo:hi], imgs, w, probs_dtype=probs_dtype, sensor_depths=s, **gates)

        # (every image is checked before the first chunk is fused)
        if labels and not all(plain):
            if m is not None and self.classes > 65535:
                raise ValueError("%s: label_map= / palette= need an aggregator of at most 65535 classes" % what)
            for i in range(n):
                if plain[i] or m is not None:
                    continue
                dt = np.dtype(getattr(images[i], "dtype", None) or np.asarray(images[i]).dtype)
                if dt.kind not in "iu":
                    raise ValueError("label image %d must have an integer dtype, got %s" % (i, dt))
                if dt.kind == "u" and np.iinfo(dt).max < self.classes:
                    raise ValueError("label image %d: %s has no value left for don't care beside %d classes" % (i, dt, self.classes))
        parts = [call(0, n, images, wts, sensors, True)] if all(plain) else []      # (nothing to undistort: the plain call)
        for lo in ([] if parts else range(0, n, GROUP_VIEWS)):
            hi = min(lo + GROUP_VIEWS, n)
            imgs, w, s = list(images[lo:hi]), None if wts is None else list(wts[lo:hi]), None if sensors is None else list(sensors[lo:hi])
            for j, i in enumerate(range(lo, hi)):
                if plain[i]:
                    continue
                cam = cameras[i]
                if labels:
                    src = images[i] if m is None else prepare_labels_device(images[i], self.classes, None, None, lmap, self.device, table)
                    dt = np.dtype(src.dtype)
                    imgs[j] = _undistort_pixels(src, cam, -1 if dt.kind == "i" else np.iinfo(dt).max, self.device, "label image %d" % i, hold=self._hold)
                    if w is not None and isinstance(w[j], np.ndarray):      # the caller's host weights go where the undistorted plane lives
                        w[j] = to_device(np.ascontiguousarray(w[j], dtype=np.float32), self.device)
                else:
                    imgs[j], wj, _ = _undistort_probs(images[i], cam, None, probs_dtype, None if wts is None else wts[i], True, False, self.device,
                                                      hold=self._hold)
                    if w is None:
                        w = [None] * (hi - lo)
                    w[j] = wj
                if s is not None:
                    s[j] = _undistort_pixels(sensors[i], cam, 0, self.device, "sensor depth image %d" % i, hold=self._hold)
            a = 0
            for b in range(1, hi - lo + 1):      # runs of consecutive views that were, or were not, undistorted
                if b == hi - lo or plain[lo + b] != plain[lo + a]:
                    through = plain[lo + a]
                    wr = None if (w is None or (through and wts is None)) else w[a:b]
                    parts.append(call(lo + a, lo + b, imgs[a:b], wr, None if s is None else s[a:b], through))
                    a = b
        parts = [p for p in parts if p is not None]
        if not parts:
            return None
        if isinstance(parts[0], tuple):
            merged = tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))
            return tuple(c[0] for c in merged) if single else merged
        merged = np.concatenate(parts)
        return merged[0] if single else merged

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        self._pending = []      # (views nobody can ask the result of any more)
        if h is not None and h.value:
            try:
                _lib.lib().smesh_aggregator_destroy(h)      # (waits for the device: every outstanding token is done afterwards)
                done = ctypes.c_int(0)
                for tok, _ in getattr(self, "_inflight", []):
                    _lib.lib().smesh_token_done(self.device, ctypes.c_uint64(tok), ctypes.byref(done))   # hands the event back to the pool
                self._inflight = []
            except Exception:
                pass

    def add(self, primitive_image, probs_image, weights_image=None, probs_dtype=None, resize=None, sample_in_kernel=False):
        """Fuse one view: `primitive_image` (W,H) of uint32/int32/uint64/int64, `probs_image` (W,H,C) float32, float16 or bfloat16,
        optional `weights_image` (W,H) float32; host numpy or device arrays, any non-negative strides.  A 16-bit image gives what
        its exactly widened float32 copy gives, without that copy (include/smesh_half.h); `probs_dtype="bfloat16"` says that a
        uint16 array holds bfloat16 bits (see `probs_code`), None infers the dtype from the array.  `resize="bilinear"`: a
        `probs_image` (w,h,C) at the network's resolution is resampled to the index image's (W,H) on the device first (`_resampled`,
        DESIGN.md 3.8); the weights image stays (W,H).  With `resize=None` such an image is refused.
        `sample_in_kernel=True` (with `resize="bilinear"` only): the small image is not resampled beforehand -- the fusion kernel
        samples it for the visible pixels (include/smesh_sampled.h), the same sums, and no (W,H,C) image exists.  The
        caller-owned small image cannot wait for a deferred group, so such an add() first hands over the views already pending and
        is then one library call and one fusion launch of its own; `fuse_views` with the keyword is the fast form."""
        from .resize import resize_mode
        mode = resize_mode(resize)
        smode = self._sampling_mode(resize, sample_in_kernel, "add")
        if type(primitive_image).__name__ == "PyCapsule":
            # render() in capsule mode (the reference's return type) handed straight back, as python/scripts/colorize_cityscapes_mesh.py:65-67 does
            from . import dlpack
            own = dlpack.own_capsule_owner(primitive_image)
            if own is not None:
                primitive_image = own
        if smode is not None:
            return self._add_sampled(primitive_image, probs_image, weights_image, probs_dtype, smode)
        if mode is not None:
            tshape = tuple(getattr(primitive_image, "shape", None) or np.shape(primitive_image))
            if len(tshape) == 2:      # (anything else is refused below, as without the keyword)
                probs_image = self._resampled(probs_image, tshape, mode, probs_dtype)
        lazy = getattr(primitive_image, "unrun", False) and primitive_image._which == 0 and primitive_image.device == self.device
        dcode = self._deferrable(probs_image, weights_image, *primitive_image.shape, probs_dtype=probs_dtype) if lazy else None
        if dcode is not None:
            # render()'s index plane handed straight back, not rasterised yet (render.py: _LazyPlane): nobody has looked at it, so
            # (camera, probs) joins the aggregator's group of deferred views and the plane is never produced
            pend = primitive_image._pending
            if pend.W and pend.H:
                self._defer(pend.renderer, pend.pod, pend.W, pend.H, probs_image, weights_image, code=dcode)
            return
        streams = []   # streams of other frameworks whose device arrays this call reads (ordered before and after, no host wait)
        if isinstance(probs_image, np.ndarray):
            probs_code(probs_image.dtype, probs_image, probs_dtype)      # (a refused probs_dtype leaves a lazy plane lazy)
        ip, imem, ishape, idt, istr, k0 = describe(primitive_image, 2, "primitive image", self.device, streams)
        pp, pmem, pshape, pdt, pstr, k1 = describe(probs_image, 3, "probs image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        code = probs_code(pdt, k1, probs_dtype)
        if code in (_lib.PROBS_F16, _lib.PROBS_BF16):
            pass      # (read as it is: smesh_aggregator_add_probs16 below)
        elif pdt != np.float32:
            if pmem == _lib.MEM_HOST and pdt.kind == "f":
                probs_image = np.asarray(probs_image, dtype=np.float32)
                pp, pmem, pshape, pdt, pstr, k1 = describe(probs_image, 3, "probs image", self.device, streams)
            else:
                raise ValueError("probs image must be float32, got %s" % pdt)
        wp, wmem, wstr, k2, wshape = None, _lib.MEM_HOST, None, None, None
        if weights_image is not None:
            wp, wmem, wshape, wdt, wstr, k2 = describe(weights_image, 2, "weights image", self.device, streams)
            if wdt != np.float32:
                if wmem == _lib.MEM_HOST and wdt.kind == "f":
                    weights_image = np.asarray(weights_image, dtype=np.float32)
                    wp, wmem, wshape, wdt, wstr, k2 = describe(weights_image, 2, "weights image", self.device, streams)
                else:
                    raise ValueError("weights image must be float32, got %s" % wdt)
        if tuple(ishape) != tuple(pshape[:2]) or (wshape is not None and tuple(wshape) != tuple(ishape)):
            # Mesh.h:68-74 std::invalid_argument
            raise ValueError("Primitive image %s, probs image %s and weights image %s must have the same width and height"
                             % (tuple(ishape), tuple(pshape[:2]), None if wshape is None else tuple(wshape)))
        if pshape[2] != self.classes:
            raise ValueError("probs image has %d classes, aggregator was built for %d" % (pshape[2], self.classes))
        W, H = ishape
        if W == 0 or H == 0:
            return
        rb = getattr(primitive_image, "_rendered_by", None)
        if code in (_lib.PROBS_F16, _lib.PROBS_BF16):
            # float16 / bfloat16 class vectors: the untouched output of renderer.render() takes the 16-bit triangle-order kernel (the
            # library re-checks that it is the latest render); everything else is widened on the device and takes add()'s path
            if not (rb is not None and not primitive_image._exported and getattr(rb, "_h", None) is not None and rb._h.value
                    and rb.device == self.device):
                rb = None
            _lib.check(_lib.lib().smesh_aggregator_add_probs16(
                self._h, None if rb is None else rb._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
                ctypes.c_void_p(pp), code, _c64(pstr), pmem,
                None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H))
            release_to(self.device, streams)
            self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if pmem == _lib.MEM_DEVICE else None,
                        k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])
            return
        if (rb is not None and not primitive_image._exported and getattr(rb, "_h", None) is not None and rb._h.value
                and idt == np.uint32 and tuple(istr) == (H, 1)):
            # the untouched output of renderer.render(): the reference's two-call loop (colorize_cityscapes_mesh.py:65-67)
            # runs the same triangle-order fusion as fuse_view (the library re-checks that it is the latest render)
            _lib.check(_lib.lib().smesh_aggregator_add_rendered(
                self._h, rb._h, ctypes.c_void_p(ip), ctypes.c_void_p(pp), _c64(pstr), pmem,
                None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H))
            release_to(self.device, streams)
            self._hold([k1 if pmem == _lib.MEM_DEVICE else None, k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])
            return
        if idt.itemsize == 4 and tuple(istr) == (H, 1) and self.match_renders and not self._records_from_image():
            # An index image that went through another framework or numpy (DLPack -> TF -> .numpy() -> add in the reference's
            # harness, eval-scannet/eval_scannet.py:211-238): if its content checksum still equals that of one of the last renders of
            # a renderer with this many primitives on this GPU, the triangle-order fusion applies (smesh_aggregator_add_matched)
            from .render import _live_renderers
            for rb in list(_live_renderers):
                if rb.device != self.device or rb._h is None or not rb._h.value or rb.getPrimitivesNum() != self.primitives:
                    continue
                matched = ctypes.c_int(0)
                _lib.check(_lib.lib().smesh_aggregator_add_matched(
                    self._h, rb._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem, ctypes.c_void_p(pp), _c64(pstr), pmem,
                    None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H, ctypes.byref(matched)))
                if matched.value:
                    release_to(self.device, streams)
                    self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if pmem == _lib.MEM_DEVICE else None,
                                k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])
                    return
        # Host images are consumed before the call returns (Fusion.h:45-47).  Device images are read asynchronously: this library's own
        # DeviceArrays are freed behind its streams, other frameworks' streams are put behind the reads by release_to() -- so the
        # record passes of the next add() on a foreign image can run beside this call's fusion (fusion.hip, add_device).
        _lib.check(_lib.lib().smesh_aggregator_add_async(
            self._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
            ctypes.c_void_p(pp), _c64(pstr), pmem,
            None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H))
        release_to(self.device, streams)
        self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if pmem == _lib.MEM_DEVICE else None,
                    k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])

    # ---- label images (include/smesh_labels.h): what the reference's colorize_mesh.py:39-67 fuses after tf.one_hot -----------------
    def _describe_labels(self, label_image, W, H, what, streams):
        """(pointer, memkind, dtype code, element strides, keep-alive) of a (W,H) label image; a host image is narrowed first."""
        lp, lmem, lshape, ldt, lstr, keep = describe(label_image, 2, what, self.device, streams)
        if ldt.name not in _lib.LBL_CODES:
            raise ValueError("%s dtype must be one of %s, got %s" % (what, "/".join(_lib.LBL_CODES), ldt))
        if (W, H) != (None, None) and tuple(lshape) != (W, H):
            raise ValueError("%s must be (W,H) = %s, got %s" % (what, (W, H), tuple(lshape)))
        if lmem == _lib.MEM_HOST and not (ldt == np.uint8 or (ldt == np.uint16 and self.classes > 255)):
            # (a uint8 image -- or a uint16 one that cannot be made narrower -- crosses PCIe as it is: the kernels treat label >= C
            # as don't-care, and the library narrows a strided one on the device)
            keep = narrow_labels(np.asarray(keep), self.classes)      # (describe() left a numpy array: only the narrow plane crosses PCIe)
            lp, lmem, lshape, ldt, lstr, keep = describe(keep, 2, what, self.device, streams)
        return lp, lmem, _lib.LBL_CODES[ldt.name], lstr, keep, tuple(lshape)

    def _describe_weights(self, weights_image, streams):
        wp, wmem, wshape, wdt, wstr, k2 = describe(weights_image, 2, "weights image", self.device, streams)
        if wdt != np.float32:
            if wmem == _lib.MEM_HOST and wdt.kind == "f":
                wp, wmem, wshape, wdt, wstr, k2 = describe(np.asarray(weights_image, dtype=np.float32), 2, "weights image", self.device, streams)
            else:
                raise ValueError("weights image must be float32, got %s" % wdt)
        return wp, wmem, tuple(wshape), wstr, k2

    # ---- label images at their own resolution and in the dataset's ids (include/smesh_label_prep.h) ---------------------------------
    @staticmethod
    def _shape_of(image):
        return tuple(getattr(image, "shape", None) or np.shape(image))

    def _prep_weights(self, weights_image, W, H, lmem, streams, what="weights image"):
        """(pointer or None, keep-alive) of the weights of a prepared fuse_view(s)_labels call: dense float32 (W,H) where the labels are."""
        if weights_image is None:
            return None, None
        wp, wmem, wshape, wstr, k2 = self._describe_weights(weights_image, streams)
        if wshape != (W, H) or wstr != (H, 1) or wmem != lmem:
            raise ValueError("%s must be contiguous float32 (W,H) in the same memory as the labels" % what)
        return wp, k2

    def _add_labels_prepared(self, primitive_image, label_image, weights_image, mode, m):
        """`add_labels(..., resize=, label_map=)` with a map or a label image of another size: the views already deferred are handed
        over first (the order of additions stays the caller's), then this view is one library call -- a render() plane that has not
        been rasterised yet is never produced (`smesh_fuse_view_labels_prepared` with its camera), any other index image goes to
        `smesh_aggregator_add_labels_prepared`.  Returns False for a call that needs no preparation (equal sizes, no map)."""
        ishape = self._shape_of(primitive_image)
        if m is None and self._shape_of(label_image) == ishape:
            return False
        streams = []
        lp, lmem, (w, h), lcode, lstr, k1, ch = _describe_label_source(label_image, self.device, streams, m=m)
        wdesc = None if weights_image is None else self._describe_weights(weights_image, streams)
        if len(ishape) != 2 or (mode is None and (w, h) != ishape) or (wdesc is not None and wdesc[2] != ishape):
            raise ValueError("Primitive image %s, label image %s and weights image %s must have the same width and height"
                             % (ishape, (w, h), None if wdesc is None else wdesc[2]))
        if ishape[0] and ishape[1] and not (w and h):
            raise ValueError("an empty label image %s cannot be resampled to %s" % ((w, h), ishape))
        lazy = getattr(primitive_image, "unrun", False) and primitive_image._which == 0 and primitive_image.device == self.device
        if lazy and (wdesc is None or (wdesc[3] == (ishape[1], 1) and wdesc[1] == lmem)):
            pend = primitive_image._pending
            if pend.W and pend.H:
                self.flush()
                fn, tail = _prepared_entry("smesh_fuse_view_labels", m, w, h, ch)
                _lib.check(fn(pend.renderer._h, self._handle, ctypes.byref(pend.pod), ctypes.c_void_p(lp), lcode, _c64(lstr),
                              None if wdesc is None else ctypes.c_void_p(wdesc[0]), lmem, *tail))
                release_to(self.device, streams)
                self._hold([k1 if lmem == _lib.MEM_DEVICE else None, wdesc[4] if (wdesc is not None and wdesc[1] == _lib.MEM_DEVICE) else None])
            return True
        ip, imem, ishape, idt, istr, k0 = describe(primitive_image, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        W, H = ishape
        if W == 0 or H == 0:
            return True
        rb = getattr(primitive_image, "_rendered_by", None)
        if not (rb is not None and not primitive_image._exported and getattr(rb, "_h", None) is not None and rb._h.value
                and rb.device == self.device):
            rb = None
        wp, wmem, wstr, k2 = (None, _lib.MEM_HOST, None, None) if wdesc is None else (wdesc[0], wdesc[1], wdesc[3], wdesc[4])
        fn, tail = _prepared_entry("smesh_aggregator_add_labels", m, w, h, ch)
        _lib.check(fn(self._h, None if rb is None else rb._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
                      ctypes.c_void_p(lp), lcode, _c64(lstr), lmem,
                      None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H, *tail))
        release_to(self.device, streams)
        self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if lmem == _lib.MEM_DEVICE else None,
                    k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])
        return True

    def add_labels(self, primitive_image, label_image, weights_image=None, resize=None, label_map=None, palette=None):
        """`add(primitive_image, one_hot(label_image), weights_image)` without the one-hot: `label_image` is (W,H) of uint8 / int8 /
        uint16 / int16 / uint32 / int32 / uint64 / int64 -- a class index per pixel, host numpy or device array, any non-negative strides
        (a mask decoded as (H,W) and passed as its transposed view is fine).  `one_hot` is tf.one_hot: a label outside [0, classes),
        negative values included, is the all-zero "don't care" vector.  On the untouched index plane of `render()` (lazy or not) of a
        triangle renderer and a Sum / Summax aggregator the view takes the label kernel (one addition per visible pixel); everything
        else expands the labels on the device and takes add()'s path.  Equal to the one-hot call for finite weights (with a non-finite
        weight that call computes 0 * inf = NaN for the pixel's other classes; this one does not).

        `resize="nearest"`: a `label_image` (w,h) of another size than the index image is sampled at half-pixel centres on the device;
        `label_map`: a one-dimensional integer table, source value v becomes map[v] after sampling (`prepare_labels_device` states
        the rule).  With either in play the views already deferred are handed over first and this view is a call of its own; with
        equal sizes and no map the call is the plain one.  Without `resize` a mask of another size is refused.
        `palette` (instead of `label_map`): `label_image` is a (w,h,3) / (w,h,4) uint8 colour image, a decoded (H,W,3) PNG passed as
        `image.transpose(1, 0, 2)`; a (K,3) uint8 array (class = row), a `ColorTable`, or a `ColorRemap` that this call first updates
        with the image -- more colours than classes afterwards is a ValueError -- and that also takes a 2-D mask
        (include/smesh_label_colors.h).  A call of its own, like `label_map`."""
        mode, m = label_resize_mode(resize), _palette_or_map(palette, label_map, [label_image], self.classes, self.device)
        if type(primitive_image).__name__ == "PyCapsule":
            from . import dlpack
            own = dlpack.own_capsule_owner(primitive_image)
            if own is not None:
                primitive_image = own
        if (mode is not None or m is not None) and self._add_labels_prepared(primitive_image, label_image, weights_image, mode, m):
            return
        if (getattr(primitive_image, "unrun", False) and primitive_image._which == 0 and primitive_image.device == self.device
                and self._deferrable_labels(label_image, weights_image, *primitive_image.shape)):
            pend = primitive_image._pending      # (render()'s plane, not rasterised yet: the view joins the group, see add())
            if pend.W and pend.H:
                self._defer(pend.renderer, pend.pod, pend.W, pend.H, label_image, weights_image, labels=True)
            return
        streams = []
        ishape = tuple(getattr(primitive_image, "shape", ()))
        if len(ishape) != 2:
            ishape = tuple(np.shape(primitive_image))
        # (the label image is checked before the index plane is looked at: a refused call leaves a lazy plane lazy)
        lp, lmem, lcode, lstr, k1, lshape = self._describe_labels(label_image, None, None, "label image", streams)
        wdesc = None if weights_image is None else self._describe_weights(weights_image, streams)
        if len(ishape) == 2 and (ishape != lshape or (wdesc is not None and wdesc[2] != ishape)):
            raise ValueError("Primitive image %s, label image %s and weights image %s must have the same width and height"
                             % (ishape, lshape, None if wdesc is None else wdesc[2]))
        ip, imem, ishape, idt, istr, k0 = describe(primitive_image, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        if tuple(ishape) != lshape or (wdesc is not None and wdesc[2] != tuple(ishape)):
            raise ValueError("Primitive image %s, label image %s and weights image %s must have the same width and height"
                             % (tuple(ishape), lshape, None if wdesc is None else wdesc[2]))
        W, H = ishape
        if W == 0 or H == 0:
            return
        rb = getattr(primitive_image, "_rendered_by", None)
        if not (rb is not None and not primitive_image._exported and getattr(rb, "_h", None) is not None and rb._h.value
                and rb.device == self.device):
            rb = None
        wp, wmem, wstr, k2 = (None, _lib.MEM_HOST, None, None) if wdesc is None else (wdesc[0], wdesc[1], wdesc[3], wdesc[4])
        _lib.check(_lib.lib().smesh_aggregator_add_labels(
            self._h, None if rb is None else rb._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
            ctypes.c_void_p(lp), lcode, _c64(lstr), lmem,
            None if wp is None else ctypes.c_void_p(wp), None if wstr is None else _c64(wstr), wmem, W, H))
        release_to(self.device, streams)
        self._hold([k0 if imem == _lib.MEM_DEVICE else None, k1 if lmem == _lib.MEM_DEVICE else None,
                    k2 if (wp is not None and wmem == _lib.MEM_DEVICE) else None])

    def fuse_view_labels(self, renderer, camera, label_image, weights_image=None, resize=None, label_map=None, palette=None,
                         sensor_depth=None, depth_gate=None, depth_stats=False, view_weights=None, view_stats=False, edge_gate=None, edge_stats=False,
                         undistort=False):
        """`fuse_view(renderer, camera, one_hot(label_image), weights_image)` without the one-hot (see add_labels, also for `resize`,
        `label_map` and `palette`; see fuse_views for `sensor_depth`, `depth_gate`, `depth_stats`, `view_weights`, `view_stats`, `edge_gate`,
        `edge_stats` and `undistort`)."""
        if undistort:
            self.flush()      # (the views already deferred come first)
            return self._fuse_views_undistorted("fuse_view_labels", True, renderer, [camera], [label_image], None if weights_image is None else [weights_image],
                                                None, resize, False, label_map, palette, None if sensor_depth is None else [sensor_depth], True,
                                                depth_gate=depth_gate, depth_stats=depth_stats, view_weights=view_weights, view_stats=view_stats,
                                                edge_gate=edge_gate, edge_stats=edge_stats)
        sensors = _gate_keywords(None if sensor_depth is None else [sensor_depth], depth_gate, depth_stats, 1, False, "fuse_view_labels")
        spec = _view_keywords(renderer, view_weights, view_stats, False, "fuse_view_labels")
        edge = _edge_keywords(edge_gate, edge_stats, False, "fuse_view_labels")
        if sensors is not None or spec is not None or edge is not None:
            stats = self._fuse_views_labels_gated(renderer, [camera], [label_image], None if weights_image is None else [weights_image],
                                                  resize, label_map, palette, sensors, depth_gate, depth_stats, "fuse_view_labels", spec, view_stats, edge, edge_stats)
            return _stats_of(stats[0], stats[1], view_stats, depth_stats, single=True, edge_counts=stats[2], edge_stats=edge_stats)
        mode, m = label_resize_mode(resize), _palette_or_map(palette, label_map, [label_image], self.classes, self.device)
        W, H = camera.resolution
        if m is not None or (mode is not None and self._shape_of(label_image) != (W, H)):
            streams = []
            lp, lmem, (w, h), lcode, lstr, k1, ch = _describe_label_source(label_image, self.device, streams, m=m)
            if mode is None and (w, h) != (W, H):
                raise ValueError("%s must be (W,H) = %s, got %s" % ("label image", (W, H), (w, h)))
            if W and H and not (w and h):
                raise ValueError("an empty label image %s cannot be resampled to %s" % ((w, h), (W, H)))
            wp, k2 = self._prep_weights(weights_image, W, H, lmem, streams)
            fn, tail = _prepared_entry("smesh_fuse_view_labels", m, w, h, ch)
            _lib.check(fn(renderer._h, self._h, ctypes.byref(camera._pod), ctypes.c_void_p(lp), lcode, _c64(lstr),
                          None if wp is None else ctypes.c_void_p(wp), lmem, *tail))
            release_to(self.device, streams)
            self._hold([k1 if lmem == _lib.MEM_DEVICE else None, k2 if lmem == _lib.MEM_DEVICE else None])
            return
        if (W > 0 and H > 0 and W <= 65536 and H <= 65536 and W * H < 0x7FFFFFFF // 4 and renderer.device == self.device
                and self._deferrable_labels(label_image, weights_image, W, H)):
            self._defer(renderer, _lib.CameraPOD.from_buffer_copy(camera._pod), W, H, label_image, weights_image, labels=True)
            return
        streams = []
        lp, lmem, lcode, lstr, k1, _ = self._describe_labels(label_image, W, H, "label image", streams)
        wp, k2 = None, None
        if weights_image is not None:
            wp_, wmem, wshape, wstr, k2 = self._describe_weights(weights_image, streams)
            if wshape != (W, H) or wstr != (H, 1) or wmem != lmem:
                raise ValueError("weights image must be contiguous float32 (W,H) in the same memory as the labels")
            wp = ctypes.c_void_p(wp_)
        _lib.check(_lib.lib().smesh_fuse_view_labels(renderer._h, self._h, ctypes.byref(camera._pod), ctypes.c_void_p(lp), lcode,
                                                     _c64(lstr), wp, lmem))
        release_to(self.device, streams)
        if lmem == _lib.MEM_DEVICE:
            self._hold([k1, k2])

    def _fuse_views_labels_prepared(self, renderer, cameras, label_images, weights_images, resize, mode, m):
        """`fuse_views_labels(..., resize=, label_map=)` with a map or images of another size: every image is checked first; images
        that share size, dtype, strides and memory go to `smesh_fuse_views_labels_prepared` as one batch -- the library prepares and
        fuses them in groups of eight --, a mixed list is fused view by view."""
        n = len(cameras)
        streams, desc = [], []
        for i, cam in enumerate(cameras):
            W, H = cam.resolution
            d = _describe_label_source(label_images[i], self.device, streams, "label image %d" % i, m=m)
            if mode is None and d[2] != (W, H):
                raise ValueError("%s must be (W,H) = %s, got %s" % ("label image %d" % i, (W, H), d[2]))
            if W and H and not (d[2][0] and d[2][1]):
                raise ValueError("an empty label image %d %s cannot be resampled to %s" % (i, d[2], (W, H)))
            w = None if weights_images is None else weights_images[i]
            desc.append((d, self._prep_weights(w, W, H, d[1], streams, "weights image %d" % i)))
        first = desc[0][0]
        if not all(d[1:5] == first[1:5] and d[6] == first[6] and (dw[0] is None) == (desc[0][1][0] is None) for d, dw in desc):
            release_to(self.device, streams)
            table = m if isinstance(m, ColorTable) else None
            for i in range(n):
                self.fuse_view_labels(renderer, cameras[i], label_images[i], None if weights_images is None else weights_images[i],
                                      resize, None if table is not None else m, table)
            return
        pods = (_lib.CameraPOD * n)(*[cam._pod for cam in cameras])
        lptr = (ctypes.c_void_p * n)(*[d[0] for d, _ in desc])
        wptr = None if desc[0][1][0] is None else (ctypes.c_void_p * n)(*[dw[0] for _, dw in desc])
        fn, tail = _prepared_entry("smesh_fuse_views_labels", m, first[2][0], first[2][1], first[6])
        _lib.check(fn(renderer._h, self._h, pods, n, lptr, first[3], _c64(first[4]), wptr, first[1], *tail))
        release_to(self.device, streams)
        if first[1] == _lib.MEM_DEVICE:
            self._hold([d[5] for d, _ in desc] + [dw[1] for _, dw in desc])

    def fuse_views_labels(self, renderer, cameras, label_images, weights_images=None, resize=None, label_map=None, palette=None,
                          sensor_depths=None, depth_gate=None, depth_stats=False, view_weights=None, view_stats=False, edge_gate=None, edge_stats=False,
                          undistort=False):
        """`fuse_views` for label images, in order (see add_labels): with a triangle renderer and a Sum / Summax aggregator up to eight
        views per fusion launch, each accumulator row read and written once for all of them.  Label images that share dtype, strides
        and memory go to the library as one batch; a mixed list is fused view by view.  `resize="nearest"` / `label_map` (see
        add_labels): the fast form for masks at the network's resolution or in the dataset's ids -- images that also share their
        size are prepared and fused by the library in batches of eight.  `palette` (see add_labels): colour images; a `ColorRemap`
        is first updated with all the call's images, in their order -- their distinct colours are found on the device, eight images
        per synchronisation -- and must then hold no more colours than the aggregator has classes.
        `sensor_depths=`, `depth_gate=`, `depth_stats=`, `view_weights=`, `view_stats=`, `edge_gate=`, `edge_stats=`: see fuse_views --
        the masks are prepared in chunks of eight, then weighted and gated.  `undistort=True`: see fuse_views -- masks (and colour
        masks) are sampled nearest, with the don't-care code where the view looks past the sensor."""
        if undistort:
            return self._fuse_views_undistorted("fuse_views_labels", True, renderer, cameras, label_images, weights_images, None, resize, False,
                                                label_map, palette, sensor_depths, False, depth_gate=depth_gate, depth_stats=depth_stats,
                                                view_weights=view_weights, view_stats=view_stats, edge_gate=edge_gate, edge_stats=edge_stats)
        cameras = list(cameras)
        sensors = _gate_keywords(sensor_depths, depth_gate, depth_stats, len(cameras), False, "fuse_views_labels")
        spec = _view_keywords(renderer, view_weights, view_stats, False, "fuse_views_labels")
        edge = _edge_keywords(edge_gate, edge_stats, False, "fuse_views_labels")
        if sensors is not None or spec is not None or edge is not None:
            stats = self._fuse_views_labels_gated(renderer, cameras, label_images, weights_images, resize, label_map, palette, sensors,
                                                  depth_gate, depth_stats, "fuse_views_labels", spec, view_stats, edge, edge_stats)
            return _stats_of(stats[0], stats[1], view_stats, depth_stats, edge_counts=stats[2], edge_stats=edge_stats)
        mode, m = label_resize_mode(resize), check_label_map(label_map)
        cameras, label_images = list(cameras), list(label_images)
        n = len(cameras)
        if len(label_images) != n or (weights_images is not None and len(weights_images) != n):
            raise ValueError("fuse_views_labels needs one label image (and one weights image or None) per camera")
        if n == 0:
            check_palette(palette, m)
            return
        m = _palette_or_map(palette, m, label_images, self.classes, self.device)
        if m is not None or (mode is not None and any(self._shape_of(label_images[i]) != tuple(cam.resolution) for i, cam in enumerate(cameras))):
            return self._fuse_views_labels_prepared(renderer, cameras, label_images, weights_images, resize, mode, m)
        streams, desc = [], []
        for i, cam in enumerate(cameras):
            W, H = cam.resolution
            d = self._describe_labels(label_images[i], W, H, "label image %d" % i, streams)
            w = None if weights_images is None else weights_images[i]
            dw = None
            if w is not None:
                dw = self._describe_weights(w, streams)
                if dw[2] != (W, H) or dw[3] != (H, 1) or dw[1] != d[1]:
                    raise ValueError("weights image %d must be contiguous float32 (W,H) in the same memory as the labels" % i)
            desc.append((d, dw))
        first = desc[0][0]
        uniform = all(d[1:4] == first[1:4] and (dw is None) == (desc[0][1] is None) for d, dw in desc)
        if not uniform:
            release_to(self.device, streams)
            for i in range(n):
                self.fuse_view_labels(renderer, cameras[i], label_images[i], None if weights_images is None else weights_images[i])
            return
        pods = (_lib.CameraPOD * n)(*[cam._pod for cam in cameras])
        lptr = (ctypes.c_void_p * n)(*[d[0] for d, _ in desc])
        wptr = None if desc[0][1] is None else (ctypes.c_void_p * n)(*[dw[0] for _, dw in desc])
        _lib.check(_lib.lib().smesh_fuse_views_labels(renderer._h, self._h, pods, n, lptr, first[2], _c64(first[3]), wptr, first[1]))
        release_to(self.device, streams)
        if first[1] == _lib.MEM_DEVICE:
            self._hold([d[4] for d, _ in desc] + [dw[4] for _, dw in desc if dw is not None])

    def add_many(self, primitive_images, probs_images, weights_images=None, probs_dtype=None, resize=None, sample_in_kernel=False):
        """`add()` for a batch of views, in order (new functionality; the reference's loop adds one image per call).  Same sums as
        the calls one by one -- per accumulator row the same float32 additions in the same order -- but device-resident dense
        uint32 / int32 index images with dense float32 device class vectors, all of one size, share their kernel launches in groups
        of up to eight (`smesh_aggregator_add_many`).  Anything else in the batch is added image by image.  `resize="bilinear"`: see
        add(); the batch is worked through in chunks of eight views, so at most eight resampled images are alive at once.
        `sample_in_kernel=True`: see add(); render() planes that have not been rasterised yet go to the library as whole batches
        (`fuse_views` with their cameras), anything else view by view."""
        from .resize import resize_mode
        mode = resize_mode(resize)
        smode = self._sampling_mode(resize, sample_in_kernel, "add_many")
        prims, probs = list(primitive_images), list(probs_images)
        wts = None if weights_images is None else list(weights_images)
        n = len(prims)
        if len(probs) != n or (wts is not None and len(wts) != n):
            raise ValueError("add_many needs one probs image (and one weights image) per primitive image")
        if n == 0:
            return
        if smode is not None:
            lazy = [getattr(p, "unrun", False) and p._which == 0 and p.device == self.device and p._pending.W and p._pending.H for p in prims]
            if all(lazy) and len({id(p._pending.renderer) for p in prims}) == 1 and (wts is None or all(x is not None for x in wts)):
                cams = [_PodCamera(p._pending.pod, p._pending.W, p._pending.H) for p in prims]
                return self._fuse_views_sampled(prims[0]._pending.renderer, cams, probs, wts, probs_dtype, smode, "add_many")
            streams = []
            for i in range(n):      # (every image is checked before the first one is added)
                self._describe_sampled(probs[i], probs_dtype, streams, "probs image %d" % i)
            release_to(self.device, streams)
            for i in range(n):
                self._add_sampled(prims[i], probs[i], None if wts is None else wts[i], probs_dtype, smode)
            return
        if mode is not None:
            for lo in range(0, n, GROUP_VIEWS):
                hi = min(lo + GROUP_VIEWS, n)
                chunk = []
                for i in range(lo, hi):
                    tshape = tuple(getattr(prims[i], "shape", None) or np.shape(prims[i]))
                    chunk.append(self._resampled(probs[i], tshape, mode, probs_dtype) if len(tshape) == 2 else probs[i])
                self.add_many(prims[lo:hi], chunk, None if wts is None else wts[lo:hi], probs_dtype=probs_dtype)
            return
        codes = [_peek_code(p, probs_dtype) for p in probs]
        known = [c for c in codes if c is not None]
        if any(c != known[0] for c in known):
            raise ValueError("add_many: all probs images must have one dtype (got %s)" % ", ".join(sorted({_lib.PROBS_NAMES[c] for c in known})))
        if known and known[0] != _lib.PROBS_F32:
            # float16 / bfloat16 class vectors: view by view through add(), where render() planes that have not been rasterised yet and
            # this library's own device images gather in deferred groups of eight -- one fuse_views call per group
            for i in range(n):
                self.add(prims[i], probs[i], None if wts is None else wts[i], probs_dtype=probs_dtype)
            return
        streams, desc = [], []
        for i in range(n):
            pi = prims[i]
            if type(pi).__name__ == "PyCapsule":
                from . import dlpack
                own = dlpack.own_capsule_owner(pi)
                if own is not None:
                    pi = own
            d_i = describe(pi, 2, "primitive image", self.device, streams)
            d_p = describe(probs[i], 3, "probs image", self.device, streams)
            d_w = None if wts is None or wts[i] is None else describe(wts[i], 2, "weights image", self.device, streams)
            desc.append((d_i, d_p, d_w))
        (ip0, imem0, ishape0, idt0, istr0, _), (pp0, pmem0, pshape0, pdt0, pstr0, _), w0 = desc[0]
        uniform = idt0 in _IDX_CODES and pdt0 == np.float32 and imem0 == _lib.MEM_DEVICE and pmem0 == _lib.MEM_DEVICE
        for d_i, d_p, d_w in desc:
            uniform = (uniform and d_i[1:5] == (imem0, ishape0, idt0, istr0) and d_p[1:5] == (pmem0, pshape0, pdt0, pstr0)
                       and (d_w is None) == (w0 is None)
                       and (d_w is None or (d_w[1] == _lib.MEM_DEVICE and d_w[3] == np.float32 and tuple(d_w[2]) == tuple(ishape0) and d_w[4] == w0[4])))
        if uniform and (tuple(ishape0) != tuple(pshape0[:2]) or pshape0[2] != self.classes):
            uniform = False      # (add() raises the reference's error for the image concerned)
        if not uniform or n < 2:
            for i in range(n):
                self.add(prims[i], probs[i], None if wts is None else wts[i], probs_dtype=probs_dtype)
            return
        W, H = ishape0
        if W == 0 or H == 0:
            return
        iptr = (ctypes.c_void_p * n)(*[d[0][0] for d in desc])
        pptr = (ctypes.c_void_p * n)(*[d[1][0] for d in desc])
        wptr = None if w0 is None else (ctypes.c_void_p * n)(*[d[2][0] for d in desc])
        _lib.check(_lib.lib().smesh_aggregator_add_many(
            self._h, n, iptr, _IDX_CODES[idt0], _c64(istr0), imem0, pptr, _c64(pstr0), pmem0,
            wptr, None if w0 is None else _c64(w0[4]), _lib.MEM_DEVICE if w0 is not None else _lib.MEM_HOST, W, H))
        release_to(self.device, streams)
        self._hold([d[0][5] for d in desc] + [d[1][5] for d in desc] + [d[2][5] for d in desc if d[2] is not None])

    # class-wide switch for the content check above
    match_renders = os.environ.get("SMESH_MATCH_RENDERS", "1") != "0"

    def _records_from_image(self):
        """smesh_aggregator_add rebuilds the per-primitive records from ANY dense image (image_records.hip; every class count since
        round 3, SMESH_ADD_RECORDS_MIN_C moves the threshold) and
        runs the same triangle-order kernels as a matched render would -- without the content checksum's read-back, which costs more
        than the records do.  (Texel renderers keep the match: their records carry the texel tables.)"""
        if os.environ.get("SMESH_ADD_RECORDS") == "0" or os.environ.get("SMESH_FUSE") == "strip":
            return False
        from .render import _live_renderers
        if any(getattr(rb, "is_texel", False) and rb.getPrimitivesNum() == self.primitives for rb in list(_live_renderers)):
            return False
        return self.classes >= int(os.environ.get("SMESH_ADD_RECORDS_MIN_C", "0"))

    def reset(self):
        with self._pending_lock:
            self._pending = []          # (deferred views whose sums would be cleared anyway)
            _lib.check(_lib.lib().smesh_aggregator_reset(self._handle))
        self._drain()

    def get(self):
        """Normalised per-primitive class distribution, fresh float32[P,C] numpy array (Fusion.h:72-76)."""
        out = result_empty((self.primitives, self.classes), np.float32)
        if out.size:
            _lib.check(_lib.lib().smesh_aggregator_get(self._h, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        self._drain()     # (get() waited for the stream: every earlier call's reads are over)
        return out

    def _labels(self, dont_care_threshold, on_device):
        if on_device:
            from .device import DeviceBuffer
            out = DeviceBuffer(max(self.primitives * 4, 4), self.device).view((self.primitives,), np.int32)
            ptr, mem = ctypes.c_void_p(out.ptr), _lib.MEM_DEVICE
        else:
            out = np.empty(self.primitives, np.int32)
            ptr, mem = out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST
        # (`_h`: the deferred views are handed to the library first, as get() does)
        _lib.check(_lib.lib().smesh_aggregator_labels(self._h, float(dont_care_threshold), ptr, mem))
        self._drain()
        return out

    def labels(self, dont_care_threshold=0.9):
        """int32 [P]: per primitive, the class with the largest value of `get()` (the lowest one among equals), -1 where the row's
        float32 sum, taken in ascending class order, is below `dont_care_threshold`.  No [P,C] array leaves the device."""
        return self._labels(dont_care_threshold, False)

    def labels_device(self, dont_care_threshold=0.9):
        """`labels()` left in HBM: a `DeviceArray` in a fresh allocation owned by the returned object -- what
        `ConfusionMatrix.add_views` / `add_image` take as their label table."""
        return self._labels(dont_care_threshold, True)

    def get_rows(self, row_lo, row_hi):
        """`get()` for the rows [row_lo, row_hi) only (row_lo a multiple of 4): what a rank owns after
        `Communicator.reduce_scatter` (new functionality)."""
        row_lo, row_hi = int(row_lo), int(row_hi)
        out = result_empty((max(row_hi - row_lo, 0), self.classes), np.float32)
        _lib.check(_lib.lib().smesh_aggregator_get_rows(self._h, row_lo, row_hi, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return out

    def get_device(self):
        """`get()` without the trip to the host: the normalised float32[P,C] result as a device-resident `DeviceArray`
        (`__cuda_array_interface__` / DLPack) in a fresh HBM allocation owned by the returned object."""
        from .device import DeviceBuffer
        buf = DeviceBuffer(max(self.primitives * self.classes * 4, 4), self.device)
        if self.primitives * self.classes:
            _lib.check(_lib.lib().smesh_aggregator_get(self._h, ctypes.c_void_p(buf.ptr), _lib.MEM_DEVICE))
        return buf.view((self.primitives, self.classes), np.float32)

    # ---- new functionality: raw accumulator access for the cross-GPU sum ----------
    def get_raw(self):
        out = np.empty((self.primitives, self.classes), np.float32)
        if out.size:
            _lib.check(_lib.lib().smesh_aggregator_get_raw(self._h, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return out

    def set_raw(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        if raw.shape != (self.primitives, self.classes):
            raise ValueError("raw accumulator must be float32[%d,%d]" % (self.primitives, self.classes))
        if raw.size:
            _lib.check(_lib.lib().smesh_aggregator_set_raw(self._h, raw.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))

    def raw_device_array(self, padded=False):
        """The un-normalised accumulator in HBM (a view, not a copy).  Rows are padded to `row_stride`
        floats in device memory: by default a strided (P,C) view is returned; `padded=True` gives the flat
        float32[P*row_stride] buffer (padding is zero), which is what an in-place all-reduce sums."""
        p, n, s = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        _lib.check(_lib.lib().smesh_aggregator_raw_pointer(self._h, ctypes.byref(p), ctypes.byref(n)))
        _lib.check(_lib.lib().smesh_aggregator_row_stride(self._h, ctypes.byref(s)))
        if padded:
            return DeviceArray(p.value, (int(n.value),), np.float32, self.device, owner=self)
        return DeviceArray(p.value, (self.primitives, self.classes), np.float32, self.device,
                           strides=(int(s.value), 1), owner=self)

    def renderer(self):
        """`ModelAggregator::renderer()` (Mesh.h:124-129): snapshot of the fused annotations for image gathers."""
        return ModelRenderer(self)

    def fuse_view(self, renderer, camera, probs_image, weights_image=None, probs_dtype=None, resize=None, sample_in_kernel=False,
                  sensor_depth=None, depth_gate=None, depth_stats=False, view_weights=None, view_stats=False, edge_gate=None, edge_stats=False,
                  undistort=False):
        """render(camera) + add(indices, probs) in one call without the indices leaving the device.  `probs_image`: contiguous (W,H,C)
        float32, float16 or bfloat16 (see add()); with `resize="bilinear"` any (w,h,C) image add() takes, resampled to the camera's
        resolution on the device first -- or, with `sample_in_kernel=True`, sampled inside the fusion kernel (see add(); one library
        call per view, after the views already deferred).  `sensor_depth=`, `depth_gate=`, `depth_stats=`: the view is gated by its
        sensor depth (see fuse_views); the views already deferred are handed over first, then this view is a call of its own.
        `view_weights=`, `view_stats=`, `edge_gate=`, `edge_stats=`: the view is weighted by its viewing geometry, gated at its
        occlusion edges (see fuse_views), under the same rule for deferred views.  `undistort=True`: `camera` is a `data.LensCamera` and
        the images are on its sensor grid (see fuse_views); the views already deferred are handed over first."""
        from .resize import resize_mode
        if undistort:
            self.flush()
            return self._fuse_views_undistorted("fuse_view", False, renderer, [camera], [probs_image], None if weights_image is None else [weights_image],
                                                probs_dtype, resize, sample_in_kernel, None, None, None if sensor_depth is None else [sensor_depth], True,
                                                depth_gate=depth_gate, depth_stats=depth_stats, view_weights=view_weights, view_stats=view_stats,
                                                edge_gate=edge_gate, edge_stats=edge_stats)
        sensors = _gate_keywords(None if sensor_depth is None else [sensor_depth], depth_gate, depth_stats, 1, sample_in_kernel, "fuse_view")
        spec = _view_keywords(renderer, view_weights, view_stats, sample_in_kernel, "fuse_view")
        edge = _edge_keywords(edge_gate, edge_stats, sample_in_kernel, "fuse_view")
        if sensors is not None or spec is not None or edge is not None:
            stats = self._fuse_views_probs_gated(renderer, [camera], [probs_image], None if weights_image is None else [weights_image],
                                                 probs_dtype, resize, sensors, depth_gate, depth_stats, "fuse_view", spec, view_stats, edge, edge_stats)
            return _stats_of(stats[0], stats[1], view_stats, depth_stats, single=True, edge_counts=stats[2], edge_stats=edge_stats)
        smode = self._sampling_mode(resize, sample_in_kernel, "fuse_view")
        if smode is not None:
            return self._fuse_views_sampled(renderer, [camera], [probs_image], None if weights_image is None else [weights_image],
                                            probs_dtype, smode, "fuse_view")
        W, H = camera.resolution
        probs_image = self._resampled(probs_image, (W, H), resize_mode(resize), probs_dtype)
        dcode = None
        if W > 0 and H > 0 and W <= 65536 and H <= 65536 and W * H < 0x7FFFFFFF // 4 and renderer.device == self.device:
            dcode = self._deferrable(probs_image, weights_image, W, H, probs_dtype=probs_dtype)
        if dcode is not None:
            self._defer(renderer, _lib.CameraPOD.from_buffer_copy(camera._pod), W, H, probs_image, weights_image, code=dcode)
            return
        streams = []
        pp, pmem, pshape, pdt, pstr, k1 = describe(probs_image, 3, "probs image", self.device, streams)
        code = probs_code(pdt, k1, probs_dtype)
        if tuple(pshape) != (W, H, self.classes) or code is None:
            raise ValueError("probs image must be float32, float16 or bfloat16 (W,H,C) = %s" % ((W, H, self.classes),))
        if pstr != (H * self.classes, self.classes, 1):
            raise ValueError("fuse_view needs a contiguous (W,H,C) probs image")
        wp = None
        if weights_image is not None:
            wp_, wmem, wshape, wdt, wstr, k2 = describe(weights_image, 2, "weights image", self.device, streams)
            if tuple(wshape) != (W, H) or wdt != np.float32 or wstr != (H, 1) or wmem != pmem:
                raise ValueError("weights image must be contiguous float32 (W,H) in the same memory as probs")
            wp = ctypes.c_void_p(wp_)
        if code != _lib.PROBS_F32:
            _lib.check(_lib.lib().smesh_fuse_view_probs16(renderer._h, self._h, ctypes.byref(camera._pod), ctypes.c_void_p(pp), code, wp, pmem))
        else:
            _lib.check(_lib.lib().smesh_fuse_view(renderer._h, self._h, ctypes.byref(camera._pod), ctypes.c_void_p(pp), wp, pmem))
        release_to(self.device, streams)
        if pmem == _lib.MEM_DEVICE:
            self._hold([k1, k2 if weights_image is not None else None])

    def _marshal_views(self, cameras, probs_images, weights_images, what, probs_dtype=None):
        """ctypes arguments of a batch of views: (pods, n, probs pointers, weights pointers or None, memory kind, keep-alives, streams,
        SMESH_PROBS_* code of the class vectors -- one dtype for the whole batch)."""
        cameras, probs_images = list(cameras), list(probs_images)
        n = len(cameras)
        if len(probs_images) != n or (weights_images is not None and len(weights_images) != n):
            raise ValueError("%s needs one probs image (and one weights image or None) per camera" % what)
        pods = (_lib.CameraPOD * max(n, 1))()
        pptr, wptr = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
        keep, mem, streams, code = [], None, [], None
        for i, cam in enumerate(cameras):
            W, H = cam.resolution
            pods[i] = cam._pod
            pp, pmem, pshape, pdt, pstr, k1 = describe(probs_images[i], 3, "probs image", self.device, streams)
            ci = probs_code(pdt, k1, probs_dtype, "probs image %d" % i)
            if tuple(pshape) != (W, H, self.classes) or ci is None:
                raise ValueError("probs image %d must be float32, float16 or bfloat16 (W,H,C) = %s" % (i, (W, H, self.classes)))
            if code is None:
                code = ci
            if ci != code:
                raise ValueError("%s: all probs images must have one dtype (image 0 is %s, image %d is %s)"
                                 % (what, _lib.PROBS_NAMES[code], i, _lib.PROBS_NAMES[ci]))
            if pstr != (H * self.classes, self.classes, 1):
                raise ValueError("%s needs contiguous (W,H,C) probs images" % what)
            if mem is None:
                mem = pmem
            if pmem != mem:
                raise ValueError("%s: all images must live in the same memory (host or device)" % what)
            pptr[i] = pp
            keep.append(k1)
            w = None if weights_images is None else weights_images[i]
            if w is not None:
                wp_, wmem, wshape, wdt, wstr, k2 = describe(w, 2, "weights image", self.device, streams)
                if tuple(wshape) != (W, H) or wdt != np.float32 or wstr != (H, 1) or wmem != mem:
                    raise ValueError("weights image %d must be contiguous float32 (W,H) in the same memory as probs" % i)
                wptr[i] = wp_
                keep.append(k2)
        return (pods, n, pptr, (None if weights_images is None else wptr), (mem if mem is not None else _lib.MEM_HOST), keep, streams,
                _lib.PROBS_F32 if code is None else code)

    def fuse_views(self, renderer, cameras, probs_images, weights_images=None, probs_dtype=None, resize=None, sample_in_kernel=False,
                   sensor_depths=None, depth_gate=None, depth_stats=False, view_weights=None, view_stats=False, edge_gate=None, edge_stats=False,
                   undistort=False):
        """`fuse_view` for a whole batch, in order (the loop of colorize_cityscapes_mesh.py:54-67 as one call).  With a
        triangle renderer and device-resident images the library rasterises and fuses up to eight views per launch: each
        accumulator row is read and written once for all of them.  All images must live in the same memory (host or device) and
        have one dtype: float32, float16 or bfloat16 (see add()).  `resize="bilinear"`: images at the network's resolution are
        resampled to their camera's on the device (see add()); when any image of the batch needs that, the batch is worked through in
        chunks of eight views -- the views of a fusion launch -- so at most eight resampled images are alive at once.  Same views in
        the same order: the same sums.  `sample_in_kernel=True` (with `resize="bilinear"`): the small images go to the library as
        they are, as one batch; the fusion kernel samples them for the visible pixels (include/smesh_sampled.h) -- the same sums,
        no (W,H,C) image anywhere.  This is the fast form of the keyword.
        `sensor_depths=` (one (w,h) uint16 / float32 sensor depth image per camera, host or device, a decoded (h,w) image as its
        transposed view) together with `depth_gate=` (a `DepthGate`): every pixel's contribution is gated by the consistency of the
        rendered depth with the sensor's (include/smesh_depth.h) -- the weights are computed on the device between the rasteriser
        and the fusion launch, eight views per launch, multiplied into `weights_images` where given.  The batch is worked through
        in chunks of eight views; host images are copied to the device per chunk.  `depth_stats=True` returns the uint64 [n, 4]
        counts [visible, far, missing, inconsistent] per view and waits for them.  Not with `sample_in_kernel=True`.
        `view_weights=` (a `ViewWeights`): every pixel's contribution is weighted by its viewing geometry -- the cosine of the angle
        between the pixel's ray and the normal of the face it shows, to an integer power, with a cut-off angle, an optional distance
        falloff and depth limit (include/smesh_view_weights.h) --, computed on the device from the render's own index and depth
        planes, eight views per launch, multiplied into `weights_images` where given; triangle renderers only.  It combines with
        everything the depth keywords combine with and with the depth keywords themselves: the view weights are computed first, the
        depth gate then gates them.  `view_stats=True` returns the uint64 [n, 4] counts [visible, far, grazing, backfacing] per view
        and waits for them; with `depth_stats=True` as well the call returns the pair (view counts, depth counts).
        `edge_gate=` (an `EdgeGate`): every pixel within a few pixels of a depth discontinuity of the render loses its weight
        (include/smesh_edge_gate.h) -- the cure for labels bleeding across occlusion edges, from the rendered depth alone, eight views
        per launch; it takes any renderer, combines with everything `view_weights=` combines with and runs between the view weights
        and the depth gate.  `edge_stats=True` returns the uint64 [n, 4] counts [visible, behind, front, silhouette] per view and
        waits; the stats asked for come back in the order (view, edge, depth), a single one bare.
        `undistort=True` (include/smesh_lens.h, lens.py): every image handed over for a `data.LensCamera` -- class vectors, and
        `sensor_depths` -- is on that lens's SENSOR grid, at any size (the network's included); the camera's pinhole part is the view
        that is rendered.  The batch is worked through in chunks of eight: each image becomes its undistorted plane on the device,
        bilinear by a rule defined to the bit, with a validity weights plane that is 0 where the view looks past the sensor (times
        `weights_images`, which stay (W,H) planes of the view); sensor depth is sampled nearest, 0 outside.  The same additions as
        fusing the planes of `undistort_probs_device` by hand, in the same order.  A plain `Camera` in the batch passes through
        untouched, and so does a lens without distortion seen through its default view at the image's size.  Not together with
        `resize=` or `sample_in_kernel=True`."""
        from .resize import image_size, resize_mode
        if undistort:
            return self._fuse_views_undistorted("fuse_views", False, renderer, cameras, probs_images, weights_images, probs_dtype, resize,
                                                sample_in_kernel, None, None, sensor_depths, False, depth_gate=depth_gate, depth_stats=depth_stats,
                                                view_weights=view_weights, view_stats=view_stats, edge_gate=edge_gate, edge_stats=edge_stats)
        cameras = list(cameras)
        sensors = _gate_keywords(sensor_depths, depth_gate, depth_stats, len(cameras), sample_in_kernel, "fuse_views")
        spec = _view_keywords(renderer, view_weights, view_stats, sample_in_kernel, "fuse_views")
        edge = _edge_keywords(edge_gate, edge_stats, sample_in_kernel, "fuse_views")
        if sensors is not None or spec is not None or edge is not None:
            stats = self._fuse_views_probs_gated(renderer, cameras, probs_images, weights_images, probs_dtype, resize, sensors, depth_gate,
                                                 depth_stats, "fuse_views", spec, view_stats, edge, edge_stats)
            return _stats_of(stats[0], stats[1], view_stats, depth_stats, edge_counts=stats[2], edge_stats=edge_stats)
        mode = resize_mode(resize)
        smode = self._sampling_mode(resize, sample_in_kernel, "fuse_views")
        if smode is not None:
            return self._fuse_views_sampled(renderer, cameras, probs_images, weights_images, probs_dtype, smode, "fuse_views")
        if mode is not None:
            cameras, probs_images = list(cameras), list(probs_images)
            wts = None if weights_images is None else list(weights_images)
            n = len(cameras)
            if len(probs_images) != n or (wts is not None and len(wts) != n):
                raise ValueError("fuse_views needs one probs image (and one weights image or None) per camera")
            if any(image_size(p) != tuple(cam.resolution) for cam, p in zip(cameras, probs_images)):
                for lo in range(0, n, GROUP_VIEWS):
                    hi = min(lo + GROUP_VIEWS, n)
                    chunk = [self._resampled(probs_images[i], tuple(cameras[i].resolution), mode, probs_dtype) for i in range(lo, hi)]
                    self.fuse_views(renderer, cameras[lo:hi], chunk, None if wts is None else wts[lo:hi], probs_dtype=probs_dtype)
                return
        pods, n, pptr, wptr, mem, keep, streams, code = self._marshal_views(cameras, probs_images, weights_images, "fuse_views", probs_dtype)
        if n == 0:
            return
        if code != _lib.PROBS_F32:
            _lib.check(_lib.lib().smesh_fuse_views_probs16(renderer._h, self._h, pods, n, pptr, code, wptr, mem))
        else:
            _lib.check(_lib.lib().smesh_fuse_views(renderer._h, self._h, pods, n, pptr, wptr, mem))
        release_to(self.device, streams)
        if mem == _lib.MEM_DEVICE:
            self._hold(keep)

    def fuse_views_ranged(self, renderer, cameras, probs_images, weights_images=None, nparts=4, on_rows=None):
        """`fuse_views` cut by accumulator row range (new functionality; `smesh_fuse_views_begin` / `_continue`): all
        views (at most 32) are rasterised, then part p = 0 .. nparts-1 fuses, for all of them in order, the triangles whose rows lie
        in one 64-row-aligned range, and `on_rows(row_lo, row_hi)` is called as soon as that part is queued -- those rows are final,
        so a sharded job exchanges them (`Communicator.allreduce_rows`) while the next part is fused.  Same sums as `fuse_views`.
        Where rows are not in triangle order (texel renderers, re-ordered meshes, host images ...) part 0 is the whole job.
        Returns the list of (row_lo, row_hi)."""
        pods, n, pptr, wptr, mem, keep, streams, code = self._marshal_views(cameras, probs_images, weights_images, "fuse_views_ranged")
        if code != _lib.PROBS_F32:
            raise ValueError("fuse_views_ranged needs float32 probs images")
        nparts = int(nparts)
        if n == 0 or nparts < 1:
            raise ValueError("fuse_views_ranged needs at least one view and nparts >= 1")
        lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
        ranges = []
        lib = _lib.lib()
        _lib.check(lib.smesh_fuse_views_begin(renderer._h, self._h, pods, n, pptr, wptr, mem, nparts, ctypes.byref(lo), ctypes.byref(hi)))
        for part in range(nparts):
            if part:
                _lib.check(lib.smesh_fuse_views_continue(renderer._h, self._h, part, ctypes.byref(lo), ctypes.byref(hi)))
            ranges.append((int(lo.value), int(hi.value)))
            if on_rows is not None and hi.value > lo.value:
                on_rows(int(lo.value), int(hi.value))
        release_to(self.device, streams)
        if mem == _lib.MEM_DEVICE:
            self._hold(keep)
        return ranges

    def get_raw_rows(self, row_lo, row_hi, plane=0):
        """Rows [row_lo, row_hi) of one plane of the raw state (plane 0: the accumulator as stored -- Mul: its hi plane, unfolded;
        plane 1: Mul's lo plane; a Mul element's value is hi + lo): float32[row_hi - row_lo, C]."""
        row_lo, row_hi = int(row_lo), int(row_hi)
        out = np.empty((max(row_hi - row_lo, 0), self.classes), np.float32)
        _lib.check(_lib.lib().smesh_aggregator_get_raw_rows(self._h, row_lo, row_hi, int(plane), out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
        return out

    def set_raw_rows(self, row_lo, raw, plane=0):
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        if raw.ndim != 2 or raw.shape[1] != self.classes:
            raise ValueError("raw rows must be float32[n,%d]" % self.classes)
        _lib.check(_lib.lib().smesh_aggregator_set_raw_rows(self._h, int(row_lo), int(row_lo) + raw.shape[0], int(plane),
                                                           raw.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))


class ModelRenderer:
    """Fused annotations gathered back to an image: `ModelAggregator::renderer()` + `ModelRenderer::render`
    (/root/reference/include/semantic_meshes/fusion/Mesh.h:124-129, 25-42).  Holds a snapshot of get()."""

    def __init__(self, aggregator):
        self.classes, self.device = aggregator.classes, aggregator.device
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_aggregator_renderer(aggregator._h, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                _lib.lib().smesh_annotation_renderer_destroy(h)
            except Exception:
                pass

    def render(self, primitive_image, background=None):
        """float32 (W,H,C) image: annotation of the primitive under each pixel, `background` (C floats,
        default zeros) where the index is out of range."""
        ip, imem, ishape, idt, istr, keep = describe(primitive_image, 2, "primitive image", self.device)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        bg = np.zeros(self.classes, np.float32) if background is None else np.ascontiguousarray(background, dtype=np.float32)
        if bg.shape != (self.classes,):
            raise ValueError("background must have %d entries" % self.classes)
        W, H = ishape
        out = np.empty((W, H, self.classes), np.float32)
        if out.size:
            _lib.check(_lib.lib().smesh_annotation_renderer_render(
                self._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem, bg.ctypes.data_as(ctypes.c_void_p),
                out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST, W, H))
        return out


    def render_device(self, primitive_image, background=None):
        """`render()` with the (W,H,C) image left in HBM: a `DeviceArray` (`__cuda_array_interface__` / DLPack) in a fresh allocation
        owned by the returned object -- what the harness's `tf.gather(annotations, idx)` (eval_scannet.py:314) produces."""
        from .device import DeviceBuffer
        ip, imem, ishape, idt, istr, keep = describe(primitive_image, 2, "primitive image", self.device)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        bg = np.zeros(self.classes, np.float32) if background is None else np.ascontiguousarray(background, dtype=np.float32)
        if bg.shape != (self.classes,):
            raise ValueError("background must have %d entries" % self.classes)
        W, H = ishape
        buf = DeviceBuffer(max(W * H * self.classes * 4, 4), self.device)
        if W * H:
            _lib.check(_lib.lib().smesh_annotation_renderer_render(
                self._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem, bg.ctypes.data_as(ctypes.c_void_p),
                ctypes.c_void_p(buf.ptr), _lib.MEM_DEVICE, W, H))
        return buf.view((W, H, self.classes), np.float32)


class MeshAggregatorSum(_MeshAggregator):
    pass


class MeshAggregatorSummax(_MeshAggregator):
    pass


class MeshAggregatorMul(_MeshAggregator):
    pass


_CLASSES = {"Sum": MeshAggregatorSum, "Summax": MeshAggregatorSummax, "Mul": MeshAggregatorMul}


def MeshAggregator(primitives, classes, aggregator="sum", images_equal_weight=0.5, device=0):
    """`semantic_meshes.fusion.MeshAggregator(primitives, classes[, aggregator[, images_equal_weight]])`
    (Fusion.cu:120-138,148-150): aggregator name is matched after capitalising its first letter."""
    name = str(aggregator)
    name = name[:1].upper() + name[1:]
    if name not in _CLASSES:
        raise ValueError("unknown aggregator %r (expected one of sum, summax, mul)" % (aggregator,))
    return _CLASSES[name](primitives, classes, name, images_equal_weight, device)


# Confusion matrices of the fused mesh against ground truth (include/smesh_eval.h)
from .evaluation import ConfusionMatrix, confusion_accuracy, confusion_iou, confusion_mean_iou  # noqa: E402,F401
from .evaluation import argmax_labels, argmax_labels_device  # noqa: E402,F401
from .label_images import LabelRenderer  # noqa: E402,F401
from .resize import resize_probs, resize_probs_device  # noqa: E402,F401
from .lens import (undistort_depth, undistort_depth_device, undistort_labels, undistort_labels_device, undistort_probs,  # noqa: E402,F401
                   undistort_probs_device)
from .mesh_results import FaceGraph, FaceSegments, PointTransfer, SurfaceIndex, VertexTransfer  # noqa: E402,F401
from .label_colors import (ColorRemap, ColorTable, check_palette, describe_color_source, resolve_palette,  # noqa: E402,F401
                           unique_colors)
