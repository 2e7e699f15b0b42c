"""Confusion matrices of the fused mesh against ground truth, counted on the device (include/smesh_eval.h).

Reference: /root/reference/eval-scannet/eval_scannet.py:108-112, 286-287 (per vertex) and :301-316 (per pixel: every frame rendered
again, `tf.gather(annotations, primitive_indices)` into a (H,W,C) float image, a confusion-matrix metric against the frame's label
image).  Here one int32 label per primitive (`MeshAggregator.labels_device()`), the rendered index plane and the ground-truth label
image give the same counts; no class-vector image is built.

A confusion matrix for C classes is uint64 [C, C + 1]: M[g, p] counts samples with ground truth g and prediction p; column C counts
DON'T-CARE predictions (a label outside [0, C), a pixel no primitive covers, an index >= P), which stay in the matrix as errors; a
sample whose ground truth is outside [0, C) enters no cell and is counted in `ignored`.  The metrics are plain numpy in float64.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, describe, release_to, to_device

_IDX_CODES = {np.dtype(np.uint32): _lib.IDX_U32, np.dtype(np.int32): _lib.IDX_I32,
              np.dtype(np.uint64): _lib.IDX_U64, np.dtype(np.int64): _lib.IDX_I64}


def _c64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _matrix(M):
    M = np.asarray(M)
    if M.ndim != 2 or M.shape[0] < 1 or M.shape[1] != M.shape[0] + 1:
        raise ValueError("a confusion matrix is [C, C + 1] (the last column counts don't-care predictions), got shape %s" % (M.shape,))
    return M.astype(np.float64), M.shape[0]


def confusion_accuracy(M):
    """trace(M[:, :C]) / M.sum(): don't-care predictions count as errors; NaN for an all-zero matrix."""
    M, C = _matrix(M)
    total = M.sum()
    return float(np.trace(M[:, :C]) / total) if total else float("nan")


def confusion_iou(M):
    """float64 [C]: M[c, c] / (M[c, :].sum() + M[:, c].sum() - M[c, c]); NaN for a class that never occurs on either side."""
    M, C = _matrix(M)
    diag = np.diagonal(M[:, :C])
    denom = M.sum(axis=1) + M[:, :C].sum(axis=0) - diag
    out = np.full(C, np.nan)
    np.divide(diag, denom, out=out, where=denom != 0)
    return out


def confusion_mean_iou(M):
    """The mean of `confusion_iou(M)` over the classes that occur; NaN when none does."""
    iou = confusion_iou(M)
    seen = ~np.isnan(iou)
    return float(iou[seen].mean()) if seen.any() else float("nan")


def lds_max_classes():
    """The class count up to which the counting kernel keeps a workgroup-private histogram in LDS (read-only library option)."""
    v = ctypes.c_int64(0)
    _lib.check(_lib.lib().smesh_get_option(b"confusion_lds_max_classes", ctypes.byref(v)))
    return int(v.value)


class ConfusionMatrix:
    """`ConfusionMatrix(classes, device=0)`: counts on `device`, read with `get()`.

    cm.add_views(renderer, cameras, labels, gt_images)   rasterise and score; no plane leaves HBM (add_view: one camera)
    cm.add_image(primitive_indices, labels, gt)          an index image from render() or from a cache
    cm.add(pred, gt)                                     1-D: per-vertex labels against per-vertex ground truth

    `labels` is int32 [P], one label per primitive (`MeshAggregator.labels()` / `labels_device()`); ground truth is any integer
    dtype, images are (W,H) -- an (H,W) array passed as its transposed view is fine.  Host numpy or device arrays.  Device inputs
    are read after a call returns: the matrix keeps them alive until `get()` or `reset()`."""

    def __init__(self, classes, device=0):
        self.classes, self.device = int(classes), int(device)
        if self.classes <= 0:
            raise ValueError("classes must be > 0")
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_confusion_create(self.classes, self.device, ctypes.byref(h)))
        self._h = h
        self._keep = []     # device inputs of calls whose kernels may still be reading them

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                _lib.lib().smesh_confusion_destroy(h)
            except Exception:
                pass

    # ---- inputs ----------------------------------------------------------------------------------------------------------------
    def _gt(self, gt, ndim, shape, what, streams):
        """(pointer, memkind, dtype code, element strides, keep-alive) of a ground-truth array; a wide host array is narrowed first."""
        ptr, mem, gshape, dt, strides, keep = describe(gt, ndim, what, self.device, streams)
        if dt.name not in _lib.LBL_CODES:
            raise ValueError("%s dtype must be one of %s, got %s" % (what, "/".join(_lib.LBL_CODES), dt))
        if tuple(gshape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(gshape)))
        if mem == _lib.MEM_HOST and self.classes <= 65535 and dt.itemsize > (1 if self.classes <= 255 else 2):
            from .fusion import narrow_labels      # (out-of-range values become 255 / 65535, which is out of range too: `ignored`)
            keep = narrow_labels(np.asarray(keep), self.classes)
            ptr, mem, gshape, dt, strides, keep = describe(keep, ndim, what, self.device, streams)
        return ptr, mem, _lib.LBL_CODES[dt.name], tuple(strides), keep

    def _labels(self, labels, what, streams, need_device):
        """(pointer, memkind, P, keep-alive) of a dense int32 [P] label table."""
        if not isinstance(labels, DeviceArray) and not hasattr(labels, "__cuda_array_interface__"):
            a = np.asarray(labels)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("%s must be an integer array [P], got %s %s" % (what, a.dtype, a.shape))
            labels = np.ascontiguousarray(a, dtype=np.int32)
            if need_device:
                labels = to_device(labels, self.device)
        ptr, mem, shape, dt, strides, keep = describe(labels, 1, what, self.device, streams)
        if dt != np.int32 or (shape[0] > 1 and strides[0] != 1):
            raise ValueError("%s must be a dense int32 array, got %s with element stride %s" % (what, dt, strides[0]))
        if need_device and mem != _lib.MEM_DEVICE:
            keep = to_device(np.ascontiguousarray(keep), self.device)
            ptr, mem = keep.ptr, _lib.MEM_DEVICE
        return ptr, mem, int(shape[0]), keep

    def _done(self, streams, keeps):
        release_to(self.device, streams)
        self._keep.extend(k for k in keeps if k is not None and not isinstance(k, np.ndarray))

    # ---- counting --------------------------------------------------------------------------------------------------------------
    def add(self, pred, gt):
        """1-D: `pred` int32 [n] predicted labels (-1 and everything else outside [0, classes): don't care), `gt` integer [n]."""
        streams = []
        pp, pmem, n, k0 = self._labels(pred, "predictions", streams, False)
        gp, gmem, gcode, gstr, k1 = self._gt(gt, 1, (n,), "ground truth", streams)
        if n > 1 and gstr[0] != 1:
            if gmem != _lib.MEM_HOST:
                raise ValueError("ground truth must be dense")
            k1 = np.ascontiguousarray(k1)
            gp = k1.ctypes.data
        _lib.check(_lib.lib().smesh_confusion_add_labels(self._h, ctypes.c_void_p(pp), pmem, ctypes.c_void_p(gp), gcode, gmem, n))
        self._done(streams, [k0, k1])

    def add_image(self, primitive_indices, labels, gt):
        """Score an index image that already exists: `primitive_indices` (W,H) of uint32 / int32 / uint64 / int64 (background and
        indices >= P: don't care), `labels` int32 [P], `gt` integer (W,H)."""
        streams = []
        ip, imem, ishape, idt, istr, k0 = describe(primitive_indices, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        lp, lmem, P, k1 = self._labels(labels, "labels", streams, False)
        gp, gmem, gcode, gstr, k2 = self._gt(gt, 2, ishape, "ground truth", streams)
        W, H = ishape
        _lib.check(_lib.lib().smesh_confusion_add_image(self._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
                                                        ctypes.c_void_p(lp), P, lmem, ctypes.c_void_p(gp), gcode, _c64(gstr), gmem, W, H))
        self._done(streams, [k0, k1, k2])

    def add_view(self, renderer, camera, labels, gt):
        """Rasterise `camera` with `renderer` and score the view against `gt` (W,H) = camera.resolution."""
        self.add_views(renderer, [camera], labels, [gt])

    def add_views(self, renderer, cameras, labels, gt_images):
        """`add_view` for a batch: up to eight views share their rasteriser launches.  Ground-truth images that share dtype, strides
        and memory go to the library as one batch; a mixed list is scored view by view."""
        cameras, gt_images = list(cameras), list(gt_images)
        n = len(cameras)
        if len(gt_images) != n:
            raise ValueError("add_views needs one ground-truth image per camera")
        streams = []
        lp, lmem, P, k0 = self._labels(labels, "labels", streams, True)
        desc = [self._gt(gt_images[i], 2, cam.resolution, "ground truth %d" % i, streams) for i, cam in enumerate(cameras)]
        runs, start = [], 0        # consecutive views whose ground truth shares dtype, strides and memory
        for i in range(1, n + 1):
            if i == n or desc[i][1:4] != desc[start][1:4]:
                runs.append((start, i))
                start = i
        if n == 0:
            runs = [(0, 0)]         # (the library still checks P and the device)
        for lo, hi in runs:
            m = hi - lo
            pods = (_lib.CameraPOD * max(m, 1))(*[cam._pod for cam in cameras[lo:hi]])
            gptr = (ctypes.c_void_p * max(m, 1))(*[d[0] for d in desc[lo:hi]])
            first = desc[lo] if m else (0, _lib.MEM_HOST, 0, (1, 1))
            _lib.check(_lib.lib().smesh_confusion_add_views(self._h, renderer._h, pods, m, ctypes.c_void_p(lp), P, gptr,
                                                            first[2], _c64(first[3]), first[1]))
        self._done(streams, [k0] + [d[4] for d in desc])

    def add_counts(self, M, ignored=0):
        """Merge a matrix counted elsewhere (another rank, another scene): uint64 [classes, classes + 1]."""
        M = np.asarray(M)
        if M.shape != (self.classes, self.classes + 1) or M.dtype.kind not in "iu" or (M.size and M.min() < 0) or int(ignored) < 0:
            raise ValueError("counts must be a non-negative integer array [%d, %d]" % (self.classes, self.classes + 1))
        M = np.ascontiguousarray(M, dtype=np.uint64)
        _lib.check(_lib.lib().smesh_confusion_add_counts(self._h, M.ctypes.data_as(ctypes.c_void_p), int(ignored)))

    def reset(self):
        _lib.check(_lib.lib().smesh_confusion_reset(self._h))
        _lib.check(_lib.lib().smesh_synchronize(self.device))      # (the inputs of earlier calls may be let go)
        self._keep = []

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def _read(self):
        M = np.zeros((self.classes, self.classes + 1), np.uint64)
        ign = ctypes.c_uint64(0)
        _lib.check(_lib.lib().smesh_confusion_get(self._h, M.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ign)))
        self._keep = []     # (get() waited for the stream: every earlier call's reads are over)
        return M, int(ign.value)

    def get(self):
        """The matrix, a fresh uint64 [classes, classes + 1] numpy array.  Waits for everything added so far."""
        return self._read()[0]

    @property
    def ignored(self):
        """Samples whose ground truth was outside [0, classes)."""
        return self._read()[1]

    def accuracy(self):
        return confusion_accuracy(self.get())

    def iou(self):
        return confusion_iou(self.get())

    def mean_iou(self):
        return confusion_mean_iou(self.get())
