"""The fused mesh rendered back into the views as label and colour images, on the device (include/smesh_label_images.h).

Reference: /root/reference/README.md step 4 ("render the annotated mesh from original camera poses to produce new 2D consistent
annotation images") and eval-scannet/eval_scannet.py:301-320: every frame rendered again, `tf.gather(annotations,
primitive_indices)` into a (H,W,C) float image, argmax, palette, `*_fused.png`.  Here one int32 label per primitive
(`MeshAggregator.labels_device()`, `VertexTransfer.labels_device()`, any integer array) and the rendered index plane give the
image at one byte per pixel (three for colours), in the (H,W) orientation image encoders take; no class-vector image is built.

For pixel (x, y) with primitive index i: l = labels[i] if 0 <= i < P, else -1 (background, negative indices, indices >= P).  If
0 <= l < classes the label is l and the colour is palette[l]; otherwise they are `dont_care_label` and `dont_care_color`.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, describe, release_to, result_empty

_IDX_CODES = {np.dtype(np.uint32): _lib.IDX_U32, np.dtype(np.int32): _lib.IDX_I32,
              np.dtype(np.uint64): _lib.IDX_U64, np.dtype(np.int64): _lib.IDX_I64}
_LAYOUTS = {"WH": _lib.LAYOUT_WH, "HW": _lib.LAYOUT_HW}


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


class LabelRenderer:
    """`LabelRenderer(labels, classes, palette=None, dont_care_label=None, dont_care_color=(0, 0, 0), dtype=None, layout="HW")`.

    lr.render_views(renderer, cameras)                 uint8 / uint16 (n,H,W): rasterise and write the label images; no plane leaves HBM
    lr.render_views_colors(renderer, cameras)          uint8 (n,H,W,3) through the palette
    lr.render_views(renderer, cameras, colors=True)    both, from one pass over each plane
    lr.render_view(renderer, camera)                   one camera: (H,W)
    lr.render_image(primitive_indices)                 an index image (W,H) that exists: render() output, a cache, any index dtype, strided

    `labels` is a SNAPSHOT taken here: int32 [P] on the device, or any 1-D integer numpy array.  `dtype=None` picks uint8 for up to
    255 classes, else uint16; `dont_care_label=None` is the dtype's maximum.  `layout="WH"` gives the project's (n,W,H[,3]) instead.
    Cameras that do not share one resolution give a list of images instead of one stacked array.  Every method has a `*_device`
    form that returns `DeviceArray`s left in HBM (asynchronous: `synchronize()`, an export or a host copy waits); device inputs
    of those are kept alive until the next call that waits."""

    def __init__(self, labels, classes, palette=None, dont_care_label=None, dont_care_color=(0, 0, 0), dtype=None, layout="HW", device=0):
        self.classes, self.device = int(classes), int(device)
        if self.classes <= 0:
            raise ValueError("classes must be > 0")
        self.dtype = np.dtype(np.uint8 if self.classes <= 255 else np.uint16) if dtype is None else np.dtype(dtype)
        if self.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError("dtype must be uint8 or uint16, got %s" % self.dtype)
        top = int(np.iinfo(self.dtype).max)
        if self.classes > top:
            raise ValueError("%d classes do not fit %s (at most %d)" % (self.classes, self.dtype, top))
        self.dont_care_label = top if dont_care_label is None else int(dont_care_label)
        if not 0 <= self.dont_care_label <= top:
            raise ValueError("dont_care_label %d does not fit %s" % (self.dont_care_label, self.dtype))
        if layout not in _LAYOUTS:
            raise ValueError("layout must be 'HW' or 'WH', got %r" % (layout,))
        self.layout = layout
        self.palette = None
        if palette is not None:
            pal = np.asarray(palette)
            if pal.dtype != np.uint8 or pal.shape != (self.classes, 3):
                raise ValueError("palette must be uint8 [%d, 3], got %s %s" % (self.classes, pal.dtype, pal.shape))
            self.palette = np.ascontiguousarray(pal)
        col = np.asarray(dont_care_color)
        if col.shape != (3,) or col.dtype.kind not in "iu" or col.min() < 0 or col.max() > 255:
            raise ValueError("dont_care_color must be three integers in [0, 255]")
        self.dont_care_color = np.ascontiguousarray(col, dtype=np.uint8)
        self._h = None
        self._host_labels = None
        self._keep = []     # device inputs of *_device calls whose kernels may still be reading them
        if isinstance(labels, DeviceArray) or hasattr(labels, "__cuda_array_interface__"):
            streams = []
            ptr, mem, shape, dt, strides, keep = describe(labels, 1, "labels", self.device, streams)
            if dt != np.int32 or (shape[0] > 1 and strides[0] != 1):
                raise ValueError("labels must be a dense int32 array, got %s with element stride %s" % (dt, strides[0]))
            self.primitives = int(shape[0])
            self._create(ptr, mem)              # a device table is resolved now: its owner may change or free it afterwards
            release_to(self.device, streams)
        else:
            a = np.asarray(labels)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("labels must be an integer array [P], got %s %s" % (a.dtype, a.shape))
            if a.dtype != np.int32:      # (whatever int32 cannot hold is no class either; unsigned tables: -1 needs a signed type)
                a = np.where((a >= 0) & (a < self.classes), a, 0).astype(np.int64) - ((a < 0) | (a >= self.classes))
            # a private copy, resolved on the device at the first use: nothing here needs a device before an image is asked for
            self._host_labels = np.array(a, dtype=np.int32, order="C", copy=True)
            self.primitives = int(self._host_labels.shape[0])

    def _create(self, ptr, mem):
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_label_renderer_create(
            ctypes.c_void_p(ptr), self.primitives, mem, self.classes, _lib.LBL_CODES[self.dtype.name], self.dont_care_label,
            None if self.palette is None else self.palette.ctypes.data_as(ctypes.c_void_p),
            self.dont_care_color.ctypes.data_as(ctypes.c_void_p), self.device, ctypes.byref(h)))
        self._h = h

    @property
    def _handle(self):
        if self._h is None:
            self._create(self._host_labels.ctypes.data, _lib.MEM_HOST)
            self._host_labels = None
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                _lib.lib().smesh_label_renderer_destroy(h)
            except Exception:
                pass

    def synchronize(self):
        """Wait for every `*_device` result so far; their device inputs are let go."""
        _lib.check(_lib.lib().smesh_synchronize(self.device))
        self._keep = []

    # ---- plumbing ----------------------------------------------------------------------------------------------------------------
    def _want(self, labels, colors):
        if colors and self.palette is None:
            raise ValueError("a colour image needs a palette")
        if not labels and not colors:
            raise ValueError("nothing to render: neither labels nor colours")

    def _shape(self, W, H, channels):
        return ((H, W) if self.layout == "HW" else (W, H)) + ((3,) if channels else ())

    def _alloc(self, shape, dtype, on_device):
        """(array, address) of an output image or batch."""
        if on_device:
            n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            out = DeviceBuffer(max(n, 4), self.device).view(shape, dtype)
            return out, out.ptr
        out = result_empty(shape, dtype)
        return out, out.ctypes.data

    def _done(self, streams, keeps, on_device):
        release_to(self.device, streams)
        if on_device:
            self._keep.extend(k for k in keeps if k is not None and not isinstance(k, np.ndarray))
        else:
            self._keep = []     # (host results: the library waited for its stream, every earlier read is over)

    def _views(self, renderer, cameras, labels, colors, on_device):
        self._want(labels, colors)
        cameras = list(cameras)
        n = len(cameras)
        sizes = [tuple(int(v) for v in cam.resolution) for cam in cameras]
        stacked = len(set(sizes)) <= 1
        W, H = sizes[0] if n else (0, 0)

        def outputs(dtype, channels):
            """(what the caller gets, [address of view i ...])"""
            if stacked:
                shape = self._shape(W, H, channels)
                out, base = self._alloc((n,) + shape, dtype, on_device)
                step = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
                return out, [base + i * step for i in range(n)]
            pairs = [self._alloc(self._shape(w, h, channels), dtype, on_device) for w, h in sizes]
            return [p[0] for p in pairs], [p[1] for p in pairs]

        lab, lptr = outputs(self.dtype, False) if labels else (None, None)
        rgb, cptr = outputs(np.uint8, True) if colors else (None, None)
        pods = (_lib.CameraPOD * max(n, 1))(*[cam._pod for cam in cameras])
        lp = None if lptr is None else (ctypes.c_void_p * max(n, 1))(*lptr)
        cp = None if cptr is None else (ctypes.c_void_p * max(n, 1))(*cptr)
        _lib.check(_lib.lib().smesh_label_renderer_render_views(self._handle, renderer._h, pods, n, _LAYOUTS[self.layout], lp, cp,
                                                                _lib.MEM_DEVICE if on_device else _lib.MEM_HOST))
        self._done([], [], on_device)
        return lab, rgb

    def _image(self, primitive_indices, labels, colors, on_device):
        self._want(labels, colors)
        streams = []
        ip, imem, ishape, idt, istr, keep = describe(primitive_indices, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        W, H = ishape
        lab, lptr = self._alloc(self._shape(W, H, False), self.dtype, on_device) if labels else (None, None)
        rgb, cptr = self._alloc(self._shape(W, H, True), np.uint8, on_device) if colors else (None, None)
        _lib.check(_lib.lib().smesh_label_renderer_render_image(
            self._handle, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem, W, H, _LAYOUTS[self.layout],
            None if lptr is None else ctypes.c_void_p(lptr), None if cptr is None else ctypes.c_void_p(cptr),
            _lib.MEM_DEVICE if on_device else _lib.MEM_HOST))
        self._done(streams, [keep], on_device)
        return lab, rgb

    @staticmethod
    def _pick(pair, labels, colors):
        return pair if labels and colors else pair[0] if labels else pair[1]

    @staticmethod
    def _first(pair):
        return tuple(None if a is None else a[0] for a in pair)

    # ---- views rasterised here -----------------------------------------------------------------------------------------------------
    def render_views(self, renderer, cameras, colors=False):
        """Label images of `cameras`: (n,H,W) of the label dtype; with `colors=True` the pair (labels, colours (n,H,W,3))."""
        return self._pick(self._views(renderer, cameras, True, colors, False), True, colors)

    def render_views_colors(self, renderer, cameras):
        """Colour images of `cameras`: uint8 (n,H,W,3)."""
        return self._views(renderer, cameras, False, True, False)[1]

    def render_view(self, renderer, camera, colors=False):
        """`render_views` for one camera: (H,W), or the pair ((H,W), (H,W,3))."""
        return self._pick(self._first(self._views(renderer, [camera], True, colors, False)), True, colors)

    def render_view_colors(self, renderer, camera):
        return self._views(renderer, [camera], False, True, False)[1][0]

    def render_views_device(self, renderer, cameras, colors=False):
        return self._pick(self._views(renderer, cameras, True, colors, True), True, colors)

    def render_views_colors_device(self, renderer, cameras):
        return self._views(renderer, cameras, False, True, True)[1]

    def render_view_device(self, renderer, camera, colors=False):
        pair = self._views(renderer, [camera], True, colors, True)
        return self._pick(tuple(None if a is None else self._slice0(a) for a in pair), True, colors)

    def render_view_colors_device(self, renderer, camera):
        return self._slice0(self._views(renderer, [camera], False, True, True)[1])

    @staticmethod
    def _slice0(a):
        """View 0 of a stacked device batch."""
        return DeviceArray(a.ptr, a.shape[1:], a.dtype, a.device, a.strides[1:], owner=a)

    # ---- an index image that exists --------------------------------------------------------------------------------------------------
    def render_image(self, primitive_indices, colors=False):
        """The label image of a (W,H) index image of uint32 / int32 / uint64 / int64, host numpy or device array, any non-negative
        strides below 2^40 elements (a render() plane that has not been rasterised yet is rasterised first); with `colors=True` the pair."""
        return self._pick(self._image(primitive_indices, True, colors, False), True, colors)

    def render_image_colors(self, primitive_indices):
        return self._image(primitive_indices, False, True, False)[1]

    def render_image_device(self, primitive_indices, colors=False):
        return self._pick(self._image(primitive_indices, True, colors, True), True, colors)

    def render_image_colors_device(self, primitive_indices):
        return self._image(primitive_indices, False, True, True)[1]
