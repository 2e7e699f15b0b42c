"""Images from cameras with lens distortion, undistorted on the device (include/smesh_lens.h).

Reference: eval-scannet/run_colmap_on_scannet.py:108 -- the reference has its users run `colmap image_undistorter` and "send all
undistorted images through your segmentation model" (README); here the images stay on the sensor's grid, at the network's
resolution if need be, and the image of the pinhole view that is rendered is built on the device, by a rule that is defined to the
bit: coordinates in double, COLMAP's polynomial model in closed form, class vectors blended as `resize=` blends
them, everything else sampled nearest.

`undistort_probs_device` / `undistort_labels_device` / `undistort_depth_device` give the planes (`undistort_probs` / `_labels` /
`_depth`: numpy copies); `MeshAggregator.fuse_view / fuse_views / fuse_view_labels / fuse_views_labels(..., undistort=True)` and
`ConfusionMatrix.add_view(s)(..., gt_undistort=True)` (fusion.py, evaluation.py) use them for every `data.LensCamera` of the call.
`add` / `add_many` / `add_labels` / `fuse_views_ranged` have no such keyword: their route is the three functions here, as
`depth_weights_device` is for the gates.  Not served: `LabelRenderer` output on the sensor's grid (that needs the iterative
inverse), the fisheye family, a group-of-eight launch, undistortion inside the fusion kernel.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, describe, release_to

_OUT_NAMES = {"float32": _lib.PROBS_F32, "float16": _lib.PROBS_F16, "bfloat16": _lib.PROBS_BF16}
_OUT_DTYPES = {_lib.PROBS_F32: np.float32, _lib.PROBS_F16: np.float16, _lib.PROBS_BF16: np.uint16}


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def lens_of(camera, what="camera"):
    """The `data.Lens` of a `data.LensCamera`; anything else is refused."""
    lens = getattr(camera, "lens", None)
    if lens is None or not hasattr(lens, "_pod"):
        raise ValueError("%s must be a data.LensCamera (a camera that carries .lens), got %r" % (what, camera))
    return lens


def is_plain(camera, size=None):
    """Does undistorting for `camera` change nothing?  A camera without a lens; or a lens whose k and p are all zero, with the default
    view, and -- where the image says its size -- an image of the view's size."""
    lens = getattr(camera, "lens", None)
    if lens is None:
        return True
    return bool(lens.is_identity and getattr(camera, "default_view", False) and tuple(camera.resolution) == lens.resolution
                and (size is None or tuple(size) == tuple(camera.resolution)))


def _finish(device, streams, mem, keep, out, hold):
    """What every call here does about a device input after its launch: see resize._resize_device."""
    release_to(device, streams)
    if mem == _lib.MEM_DEVICE:
        if isinstance(keep, DeviceArray):
            out._inputs = keep            # (the kernel may still be reading it)
        elif hold is not None:
            hold([keep])
        else:
            _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)


def _undistort_probs(image, camera, out_dtype, probs_dtype, weights_image, want_weights, want_counts, device, hold=None):
    from .evaluation import _describe_probs
    from .resize import _out_code
    lens = lens_of(camera)
    streams = []
    pp, pmem, (w, h, C), code, pstr, keep = _describe_probs(image, probs_dtype, device, streams)
    ocode = _out_code(out_dtype, code)
    W, H = camera.resolution
    if not (w and h):
        raise ValueError("an empty probs image %s cannot be undistorted" % ((w, h),))
    if isinstance(keep, DeviceArray):
        device = keep.device
    odt = _OUT_DTYPES[ocode]
    out = DeviceBuffer(max(W * H * C * np.dtype(odt).itemsize, 16), device).view((W, H, C), odt)
    out.bfloat16 = ocode == _lib.PROBS_BF16
    wout, win, wkeep = None, None, None
    if want_weights or weights_image is not None:
        wout = DeviceBuffer(max(W * H * 4, 16), device).view((W, H), np.float32)
        if weights_image is not None:
            from .fusion import _dense_plane
            win, wkeep = _dense_plane(weights_image, W, H, device, "weights image", streams)
    counts = np.zeros(2, np.uint64) if want_counts else None
    _lib.check(_lib.lib().smesh_undistort_probs(ctypes.c_void_p(pp), code, _c64(pstr), pmem, w, h, C, ctypes.byref(lens._pod), ctypes.byref(camera._pod),
                                                ctypes.c_void_p(out.ptr), ocode, None if win is None else ctypes.c_void_p(win),
                                                None if wout is None else ctypes.c_void_p(wout.ptr),
                                                None if counts is None else counts.ctypes.data_as(ctypes.c_void_p), int(device)))
    _finish(device, streams, pmem, keep, out, hold)
    if wout is not None and wkeep is not None:
        if isinstance(wkeep, DeviceArray):
            wout._inputs = wkeep
        elif hold is not None:
            hold([wkeep])
        else:
            _lib.synchronize(device)
    return out, wout, counts


def undistort_probs_device(image, camera, out_dtype=None, probs_dtype=None, weights_image=None, return_weights=False, return_counts=False,
                           device=0):
    """The class-vector image `image` (w,h,C), on the sensor grid of `camera` (a `data.LensCamera`) at any size, as the pinhole view
    of that camera sees it: a dense (W,H,C) `DeviceArray` in a fresh allocation -- float32, float16, or uint16 bit patterns with
    `.bfloat16` set; `out_dtype` None: the input's dtype.  `image`: what `MeshAggregator.add` takes (numpy, device arrays, DLPack; any
    non-negative strides); a host image crosses PCIe at its own size.  Bilinear, defined to the bit; the row of a
    view pixel that falls outside the sensor is all +0.0.  `return_weights=True` (implied by `weights_image=`): also the (W,H) float32
    validity plane -- 1, or `weights_image` (a (W,H) plane of the view), inside, 0 outside -- from the same launch; a fusion call
    given the pair adds nothing for the outside pixels.  `return_counts=True`: also the uint64 counts [pixels, outside]; the call then
    waits for them.  Returns the image, or the tuple (image[, weights][, counts])."""
    out, wout, counts = _undistort_probs(image, camera, out_dtype, probs_dtype, weights_image, return_weights, return_counts, device)
    res = (out,) + ((wout,) if wout is not None else ()) + ((counts,) if return_counts else ())
    return res[0] if len(res) == 1 else res


def undistort_probs(image, camera, out_dtype=None, probs_dtype=None, weights_image=None, return_weights=False, return_counts=False, device=0):
    """`undistort_probs_device` with the device arrays copied to numpy (bfloat16: uint16 bit patterns)."""
    res = undistort_probs_device(image, camera, out_dtype, probs_dtype, weights_image, return_weights, return_counts, device)
    if isinstance(res, tuple):
        return tuple(r.numpy() if isinstance(r, DeviceArray) else r for r in res)
    return res.numpy()


def _undistort_pixels(image, camera, fill, device, what, return_counts=False, hold=None):
    lens = lens_of(camera)
    streams = []
    ndim = getattr(image, "ndim", None)
    if ndim is None:
        image = np.asarray(image)
        ndim = image.ndim
    if ndim not in (2, 3):
        raise ValueError("%s must be (w,h) or (w,h,channels), got %d dimensions" % (what, ndim))
    ip, imem, ishape, idt, istr, keep = describe(image, ndim, what, device, streams)
    idt = np.dtype(idt)
    ch = 1 if ndim == 2 else int(ishape[2])
    if idt.kind not in "iuf" or idt.itemsize not in (1, 2, 4, 8):
        raise ValueError("%s must have integer or floating-point elements of 1, 2, 4 or 8 bytes, got %s" % (what, idt))
    if not 1 <= ch <= 4:
        raise ValueError("%s must have 1 to 4 channels, got %d" % (what, ch))
    w, h = int(ishape[0]), int(ishape[1])
    if not (w and h):
        raise ValueError("an empty %s %s cannot be undistorted" % (what, (w, h)))
    try:
        pixel = np.broadcast_to(np.asarray(fill), (ch,))
        if idt.kind in "iu" and not np.all((pixel >= np.iinfo(idt).min) & (pixel <= np.iinfo(idt).max)):
            raise ValueError
        pixel = np.ascontiguousarray(pixel.astype(idt))
    except (TypeError, ValueError):
        raise ValueError("fill must be one value, or one per channel, that %s holds; got %r" % (idt, fill))
    if isinstance(keep, DeviceArray):
        device = keep.device
    W, H = camera.resolution
    out = DeviceBuffer(max(W * H * ch * idt.itemsize, 16), device).view((W, H) if ndim == 2 else (W, H, ch), idt)
    strides = tuple(istr) + ((0,) if ndim == 2 else ())
    counts = np.zeros(2, np.uint64) if return_counts else None
    _lib.check(_lib.lib().smesh_undistort_pixels(ctypes.c_void_p(ip), idt.itemsize, ch, _c64(strides), imem, w, h, ctypes.byref(lens._pod),
                                                 ctypes.byref(camera._pod), pixel.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out.ptr),
                                                 None if counts is None else counts.ctypes.data_as(ctypes.c_void_p), int(device)))
    _finish(device, streams, imem, keep, out, hold)
    return (out, counts) if return_counts else out


def undistort_labels_device(image, camera, fill, device=0, return_counts=False):
    """The mask `image`, on the sensor grid of `camera` (a `data.LensCamera`) at any size, as the pinhole view sees it, sampled
    NEAREST: a dense `DeviceArray` (W,H) -- or (W,H,channels) for a (w,h,3) / (w,h,4) colour mask -- of the image's own dtype (any
    integer dtype).  A view pixel that falls outside the sensor gets `fill`: one value, or one per channel; choose one that the
    consumer reads as don't care.  `image`: host numpy or a device array, any non-negative strides (a decoded (h,w[,ch]) image as its
    transposed view).  `return_counts=True`: also the uint64 counts [pixels, outside]."""
    return _undistort_pixels(image, camera, fill, device, "label image", return_counts)


def undistort_labels(image, camera, fill, device=0):
    """`undistort_labels_device` copied to a numpy array."""
    return undistort_labels_device(image, camera, fill, device).numpy()


def undistort_depth_device(image, camera, device=0):
    """The sensor depth image `image` (w,h), uint16 or float32, on the sensor grid of `camera`, as the pinhole view sees it: a dense
    (W,H) `DeviceArray` of the same dtype, sampled nearest -- depth is never blended --, 0 where the view looks past the sensor: the
    depth gate's "missing" (`fusion.DepthGate`)."""
    dt = np.dtype(getattr(image, "dtype", None) or np.asarray(image).dtype)
    if dt not in (np.dtype(np.uint16), np.dtype(np.float32)) or getattr(image, "ndim", np.ndim(image)) != 2:
        raise ValueError("a sensor depth image must be uint16 or float32 (w,h), got %s" % dt)
    return _undistort_pixels(image, camera, 0, device, "sensor depth image")


def undistort_depth(image, camera, device=0):
    """`undistort_depth_device` copied to a numpy array."""
    return undistort_depth_device(image, camera, device).numpy()
