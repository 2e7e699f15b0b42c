"""Class-vector images at the network's resolution, resampled to the camera's on the device (include/smesh_resize.h).

Reference: eval-scannet/eval_scannet.py:221-236 -- the network runs at 640 x 480, `tf.image.resize(pred_probs,
resolution, method="bilinear")` makes the (968,1296,40) image that is scored and fused -- and
python/scripts/colorize_cityscapes_mesh.py:42 (`multi_scale(predictor, [0.5])`).  Here the small image is what crosses PCIe, and the
resampling is defined to the bit: half-pixel centres, no antialiasing, coordinates in double, three float32 lerps.

`resize_probs_device` / `resize_probs` give the dense (W,H,C) image; `argmax_labels(..., size=, resize=)`,
`ConfusionMatrix.add_probs(..., resize=)` and `MeshAggregator.add / add_many / fuse_view / fuse_views(..., resize=)` (evaluation.py,
fusion.py) use it where their image's width and height differ from the target's.  Nearest-neighbour resampling of class vectors
and `fuse_views_ranged` are not served.  Label images have a keyword of their own -- `resize="nearest"` on `add_labels` /
`fuse_view(s)_labels`, `gt_resize=` on `ConfusionMatrix` -- with its own rule and validation (include/smesh_label_prep.h,
`fusion.prepare_labels_device`): they are sampled, not blended.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, release_to

_OUT_NAMES = {"float32": _lib.PROBS_F32, "float16": _lib.PROBS_F16, "bfloat16": _lib.PROBS_BF16}


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def resize_mode(resize, what="resize"):
    """The SMESH_RESIZE_* code of a `resize=` keyword: None (no resampling) stays None, "bilinear" is the one mode there is."""
    if resize is None:
        return None
    if not isinstance(resize, str) or resize not in _lib.RESIZE_MODES:
        raise ValueError("%s must be None or one of %s, got %r" % (what, "/".join(sorted(_lib.RESIZE_MODES)), resize))
    return _lib.RESIZE_MODES[resize]


def target_size(size, what="size"):
    """(W, H) of a `size=` keyword: two non-negative integers."""
    try:
        W, H = size
        W, H = int(W), int(H)
    except (TypeError, ValueError):
        raise ValueError("%s must be (W, H), got %r" % (what, size))
    if W < 0 or H < 0:
        raise ValueError("%s must not be negative, got %r" % (what, (W, H)))
    return W, H


def _out_code(out_dtype, in_code):
    if out_dtype is None:
        return in_code
    name = out_dtype if isinstance(out_dtype, str) else np.dtype(out_dtype).name
    if name not in _OUT_NAMES:
        raise ValueError("out_dtype must be None, 'float32', 'float16' or 'bfloat16', got %r" % (out_dtype,))
    return _OUT_NAMES[name]


def _resize_device(probs, size, out_dtype, probs_dtype, mode, device, hold=None):
    """`resize_probs_device` after its keywords were checked.  `hold`: called with the keep-alives of a foreign device input instead
    of waiting for the device (MeshAggregator: a completion token)."""
    from .evaluation import _describe_probs
    streams = []
    pp, pmem, (w, h, C), code, pstr, keep = _describe_probs(probs, probs_dtype, device, streams)
    ocode = _out_code(out_dtype, code)
    W, H = size
    if W and H and not (w and h):
        raise ValueError("an empty probs image %s cannot be resampled to %s" % ((w, h), (W, H)))
    if isinstance(keep, DeviceArray):
        device = keep.device
    odt = {_lib.PROBS_F32: np.float32, _lib.PROBS_F16: np.float16, _lib.PROBS_BF16: np.uint16}[ocode]
    out = DeviceBuffer(max(W * H * C * np.dtype(odt).itemsize, 16), device).view((W, H, C), odt)
    out.bfloat16 = ocode == _lib.PROBS_BF16
    if W and H:
        _lib.check(_lib.lib().smesh_resize_probs(ctypes.c_void_p(pp), code, _c64(pstr), pmem, w, h, C,
                                                 ctypes.c_void_p(out.ptr), ocode, W, H, mode, int(device)))
    release_to(device, streams)
    if pmem == _lib.MEM_DEVICE:
        if isinstance(keep, DeviceArray):
            out._inputs = keep            # (the kernel may still be reading it)
        elif hold is not None:
            hold([keep])
        else:
            _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)
    return out


def resize_probs_device(probs, size, out_dtype=None, probs_dtype=None, mode="bilinear", device=0):
    """The class-vector image `probs` (w,h,C) resampled to `size` = (W,H): a dense (W,H,C) `DeviceArray`, class fastest, in a fresh
    allocation -- float32, float16, or uint16 bit patterns with `.bfloat16` set; `out_dtype` None: the input's dtype.  `probs`: what
    `MeshAggregator.add` takes (float32 / float16 / bfloat16; numpy, device arrays, DLPack; any non-negative strides -- a network's
    (h,w,C) tensor or a channel-first (C,h,w) one as its permuted view); a host image crosses PCIe at its own size.  `mode`:
    "bilinear" -- half-pixel centres, no antialiasing, defined to the bit in DESIGN.md 3.8: equal sizes give an exact copy, a 16-bit
    output is the float32 result rounded to nearest even."""
    code = resize_mode(mode, "mode")
    if code is None:
        raise ValueError("mode must be 'bilinear'")
    return _resize_device(probs, target_size(size), out_dtype, probs_dtype, code, device)


def resize_probs(probs, size, out_dtype=None, probs_dtype=None, mode="bilinear", device=0):
    """`resize_probs_device` copied to a numpy array (W,H,C) (bfloat16: uint16 bit patterns)."""
    return resize_probs_device(probs, size, out_dtype, probs_dtype, mode, device).numpy()


def image_size(obj):
    """(w, h) of a class-vector image that says its shape without being touched (numpy, DeviceArray, torch, cupy), else None -- a
    DLPack capsule is consumed by whoever looks inside."""
    shape = getattr(obj, "shape", None)
    if shape is None and isinstance(obj, (list, tuple)):
        shape = np.shape(obj)
    try:
        if shape is not None and len(shape) == 3:
            return int(shape[0]), int(shape[1])
    except TypeError:
        pass
    return None
