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
from .device import DeviceArray, DeviceBuffer, describe, release_to, to_device

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


# ---- the labels of a class-vector image (include/smesh_probs_labels.h) ---------------------------------------------------------
_OUT_DTYPES = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535, np.dtype(np.int32): 2 ** 31 - 1}


def _describe_probs(probs, probs_dtype, device, streams, what="probs image"):
    """(pointer, memkind, (W,H,C), SMESH_PROBS_* code, element strides, keep-alive) of a class-vector image: what
    `MeshAggregator.add` takes -- float32 / float16 / bfloat16, numpy, `__cuda_array_interface__` or DLPack, any non-negative strides."""
    from .fusion import probs_code
    if isinstance(probs, np.ndarray):
        probs_code(probs.dtype, probs, probs_dtype, what)       # (a refused probs_dtype is refused before anything is touched)
    pp, pmem, pshape, pdt, pstr, keep = describe(probs, 3, what, device, streams)
    code = probs_code(pdt, keep, probs_dtype, what)
    if code is None:
        if pmem == _lib.MEM_HOST and pdt.kind == "f":
            pp, pmem, pshape, pdt, pstr, keep = describe(np.asarray(keep, dtype=np.float32), 3, what, device, streams)
            code = _lib.PROBS_F32
        else:
            raise ValueError("%s must be float32, float16 or bfloat16, got %s" % (what, pdt))
    if pshape[2] < 1:
        raise ValueError("%s must have at least one class, got shape %s" % (what, tuple(pshape)))
    return pp, pmem, tuple(int(v) for v in pshape), code, tuple(pstr), keep


def _label_out(classes, dtype, dont_care_label):
    """(numpy dtype, don't-care value) of a label image for `classes` classes: uint8 up to 255 classes, else uint16, unless `dtype`
    (uint8 / uint16 / int32) says otherwise; the don't-care value defaults to the dtype's maximum and is never a class."""
    classes = int(classes)
    if dtype is None:
        if classes > 65535:
            raise ValueError("more than 65535 classes need dtype=np.int32")
        dt = np.dtype(np.uint8 if classes <= 255 else np.uint16)
    else:
        dt = np.dtype(dtype)
        if dt not in _OUT_DTYPES:
            raise ValueError("label dtype must be uint8, uint16 or int32, got %s" % dt)
    if dt != np.int32 and classes > _OUT_DTYPES[dt]:
        raise ValueError("%s is too narrow for %d classes" % (dt, classes))
    dc = _OUT_DTYPES[dt] if dont_care_label is None else int(dont_care_label)
    info = np.iinfo(dt)
    if not info.min <= dc <= info.max:
        raise ValueError("%s cannot hold the don't-care label %d" % (dt, dc))
    if 0 <= dc < classes:
        raise ValueError("the don't-care label %d is one of the %d classes" % (dc, classes))
    return dt, dc


def _threshold(dont_care_threshold):
    """None: no don't-care test (-inf: the kernel computes no sum)."""
    if dont_care_threshold is None:
        return float("-inf")
    t = float(dont_care_threshold)
    if t != t:
        raise ValueError("the don't-care threshold must not be NaN")
    return t


def _label_image_like(W, H, pstr, dt, device):
    """A fresh (W,H) device image of `dt` whose memory order follows the class-vector image's pixel order: y fastest for the dense
    (W,H,C) image, x fastest for a network's (H,W,C) tensor seen as (W,H,C)."""
    buf = DeviceBuffer(max(W * H * dt.itemsize, 1), device)
    strides = (1, W) if (W > 1 and H > 1 and pstr[0] < pstr[1]) else (H, 1)
    return DeviceArray(buf.ptr, (W, H), dt, device, strides, owner=buf)


def argmax_labels_device(probs, dont_care_threshold=None, dont_care_label=None, dtype=None, probs_dtype=None, device=0, size=None,
                         resize=None):
    """The label of every pixel of a class-vector image `probs` (W,H,C), on the device: the lowest class with the largest value (a NaN
    never replaces the current best; include/smesh_probs_labels.h), as a (W,H) `DeviceArray` of `dtype` (None: uint8 up to 255
    classes, else uint16).  With `dont_care_threshold` a pixel whose float32 class sum is below it gets `dont_care_label` (None: the
    dtype's maximum) -- what `add_labels` and `ConfusionMatrix` read as "don't care".  `probs`: what `MeshAggregator.add` takes
    (float32 / float16 / bfloat16; numpy, device arrays, DLPack; a (H,W,C) tensor as its transposed view); the result's memory order
    follows the input's pixel order.  `add_labels(idx, argmax_labels_device(probs))` is hard-vote fusion of soft predictions.
    With `size=(W,H)` and `resize="bilinear"` the labels are those of `resize_probs(probs, size)` in float32 (resize.py; DESIGN.md
    3.8) -- a dense (W,H) image, and no (W,H,C) image is built."""
    from .resize import resize_mode, target_size
    mode = resize_mode(resize)
    if (size is None) != (mode is None):
        raise ValueError("size=(W,H) and resize='bilinear' go together, got size=%r, resize=%r" % (size, resize))
    if size is not None:
        size = target_size(size)
    streams = []
    thr = _threshold(dont_care_threshold)
    pp, pmem, (W, H, C), code, pstr, keep = _describe_probs(probs, probs_dtype, device, streams)
    dt, dc = _label_out(C, dtype, dont_care_label)
    if isinstance(keep, DeviceArray):
        device = keep.device
    if mode is not None:
        w, h = W, H
        W, H = size
        if W and H and not (w and h):
            raise ValueError("an empty probs image %s cannot be resampled to %s" % ((w, h), (W, H)))
        out = DeviceBuffer(max(W * H * dt.itemsize, 1), device).view((W, H), dt)
        if W and H:
            _lib.check(_lib.lib().smesh_resize_probs_labels(ctypes.c_void_p(pp), code, _c64(pstr), pmem, w, h, C, thr,
                                                            ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], _c64(out.strides), dc,
                                                            W, H, mode, int(device)))
    else:
        out = _label_image_like(W, H, pstr, dt, device)
        if W and H:
            _lib.check(_lib.lib().smesh_probs_labels(ctypes.c_void_p(pp), code, _c64(pstr), pmem, W, H, C, thr,
                                                     ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], _c64(out.strides), dc, _lib.MEM_DEVICE,
                                                     int(device)))
    release_to(device, streams)
    if pmem == _lib.MEM_DEVICE:
        if isinstance(keep, DeviceArray):
            out._inputs = keep            # (the kernel may still be reading it)
        else:
            _lib.synchronize(device)      # (a foreign input may be freed by its owner as soon as we return)
    return out


def argmax_labels(probs, dont_care_threshold=None, dont_care_label=None, dtype=None, probs_dtype=None, device=0, size=None, resize=None):
    """`argmax_labels_device` copied to a numpy array (W,H)."""
    return argmax_labels_device(probs, dont_care_threshold, dont_care_label, dtype, probs_dtype, device, size, resize).numpy()


class ConfusionMatrix:
    """`ConfusionMatrix(classes, device=0)`: counts on `device`, read with `get()`.

    cm.add_views(renderer, cameras, labels, gt_images)   rasterise and score; no plane leaves HBM (add_view: one camera)
    cm.add_image(primitive_indices, labels, gt)          an index image from render() or from a cache
    cm.add(pred, gt)                                     1-D: per-vertex labels against per-vertex ground truth
    cm.add_probs(probs, gt)                              the network's own (W,H,C) class-vector image, arg-maxed and counted in one pass

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

    def _prepared_gt(self, gt, shape, gt_resize, gt_map, what, gt_palette=None):
        """The ground truth of a call with `gt_resize=` / `gt_map=` (include/smesh_label_prep.h, `fusion.prepare_labels_device`): `gt`
        itself where neither is in play -- no map, and its shape is `shape` (None: whatever it is) already --, else its prepared dense
        uint8 / uint16 plane on the device, which the entry points below take as they take any ground truth: every value >= classes,
        the plane's don't-care code included, enters no cell and counts in `ignored`.  `gt_palette=` (include/smesh_label_colors.h):
        `gt` is a (W,H,3) / (W,H,4) uint8 colour image, `gt_palette` a (K,3) uint8 array (class = row) or a `fusion.ColorTable` -- ground
        truth has a known palette --; a colour outside it is ignored."""
        from .fusion import check_label_map, check_palette, label_resize_mode, prepare_labels_device
        mode, m = label_resize_mode(gt_resize), check_label_map(gt_map)
        gshape = tuple(getattr(gt, "shape", None) or np.shape(gt))
        pal = check_palette(gt_palette, m, remap_ok=False, what="gt_palette")
        if pal is not None:
            if self.classes > 65535:
                raise ValueError("gt_palette needs a confusion matrix of at most 65535 classes")
            if shape is not None and mode is None and gshape[:2] != tuple(shape):
                raise ValueError("%s must have shape %s + (3 or 4,), got %s" % (what, tuple(shape), gshape))
            return prepare_labels_device(gt, self.classes, shape, gt_resize, None, self.device, pal)
        if m is None and (mode is None or shape is None or gshape == tuple(shape)):
            return gt
        if self.classes > 65535:
            raise ValueError("gt_map / gt_resize need a confusion matrix of at most 65535 classes")
        if shape is not None and mode is None and gshape != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), gshape))
        if len(gshape) == 1:
            plane = prepare_labels_device(gt, self.classes, None, None, m, self.device)
            return DeviceArray(plane.ptr, (plane.shape[0],), plane.dtype, plane.device, owner=plane)
        return prepare_labels_device(gt, self.classes, shape, gt_resize, m, self.device)

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
    def add(self, pred, gt, gt_map=None):
        """1-D: `pred` int32 [n] predicted labels (-1 and everything else outside [0, classes): don't care), `gt` integer [n].
        `gt_map`: a one-dimensional integer table, ground-truth value v counts as map[v] (outside the table: ignored)."""
        streams = []
        pp, pmem, n, k0 = self._labels(pred, "predictions", streams, False)
        gt = self._prepared_gt(gt, (n,), None, gt_map, "ground truth")
        gp, gmem, gcode, gstr, k1 = self._gt(gt, 1, (n,), "ground truth", streams)
        if n > 1 and gstr[0] != 1:
            if gmem != _lib.MEM_HOST:
                raise ValueError("ground truth must be dense")
            k1 = np.ascontiguousarray(k1)
            gp = k1.ctypes.data
        _lib.check(_lib.lib().smesh_confusion_add_labels(self._h, ctypes.c_void_p(pp), pmem, ctypes.c_void_p(gp), gcode, gmem, n))
        self._done(streams, [k0, k1])

    def add_image(self, primitive_indices, labels, gt, gt_resize=None, gt_map=None, gt_palette=None):
        """Score an index image that already exists: `primitive_indices` (W,H) of uint32 / int32 / uint64 / int64 (background and
        indices >= P: don't care), `labels` int32 [P], `gt` integer (W,H).  `gt_resize="nearest"`: a `gt` of another size is sampled
        at half-pixel centres on the device; `gt_map`: ground-truth value v counts as map[v], after sampling (the rule of
        `fusion.prepare_labels_device`; eval_scannet.py's tf.gather(scannet_to_nyu40, gt) is `gt_map=scannet_to_nyu40 - 1`).
        `gt_palette`: `gt` is a colour image (W,H,3) / (W,H,4) uint8 and counts as the class of its colour -- a (K,3) uint8 array
        (class = row) or a `fusion.ColorTable`; a colour outside the palette is ignored."""
        streams = []
        ip, imem, ishape, idt, istr, k0 = describe(primitive_indices, 2, "primitive image", self.device, streams)
        if idt not in _IDX_CODES:
            raise ValueError("primitive image dtype must be one of uint32/int32/uint64/int64, got %s" % idt)
        lp, lmem, P, k1 = self._labels(labels, "labels", streams, False)
        gt = self._prepared_gt(gt, tuple(ishape), gt_resize, gt_map, "ground truth", gt_palette)
        gp, gmem, gcode, gstr, k2 = self._gt(gt, 2, ishape, "ground truth", streams)
        W, H = ishape
        _lib.check(_lib.lib().smesh_confusion_add_image(self._h, ctypes.c_void_p(ip), _IDX_CODES[idt], _c64(istr), imem,
                                                        ctypes.c_void_p(lp), P, lmem, ctypes.c_void_p(gp), gcode, _c64(gstr), gmem, W, H))
        self._done(streams, [k0, k1, k2])

    def _undistorted_gt(self, gt, camera, gt_map, gt_palette, what):
        """Ground truth on the sensor grid of a `data.LensCamera`, at any size, as that camera's pinhole view sees it
        (include/smesh_lens.h, `fusion.undistort_labels_device`): sampled nearest, with a value no class has where the view looks past
        the sensor, so those pixels count in `ignored`.  With `gt_map` / `gt_palette` the image is first turned into classes at its
        own size -- both work pixel by pixel, so the order does not matter -- and the plane's don't-care code is the fill."""
        from .lens import _undistort_pixels, is_plain
        gshape = tuple(getattr(gt, "shape", None) or np.shape(gt))
        if is_plain(camera, gshape):
            return gt, gt_map, gt_palette
        if gt_map is not None or gt_palette is not None:
            gt = self._prepared_gt(gt, None, None, gt_map, what, gt_palette)
        dt = np.dtype(getattr(gt, "dtype", None) or np.asarray(gt).dtype)
        if dt.kind not in "iu" or (dt.kind == "u" and np.iinfo(dt).max < self.classes):
            raise ValueError("%s: %s has no value left for the pixels outside the sensor beside %d classes" % (what, dt, self.classes))
        return _undistort_pixels(gt, camera, -1 if dt.kind == "i" else np.iinfo(dt).max, self.device, what), None, None

    def add_view(self, renderer, camera, labels, gt, gt_resize=None, gt_map=None, gt_palette=None, gt_undistort=False):
        """Rasterise `camera` with `renderer` and score the view against `gt` (W,H) = camera.resolution (`gt_resize`, `gt_map`,
        `gt_palette`: see add_image; `gt_undistort`: see add_views)."""
        self.add_views(renderer, [camera], labels, [gt], gt_resize, gt_map, gt_palette, gt_undistort)

    def add_views(self, renderer, cameras, labels, gt_images, gt_resize=None, gt_map=None, gt_palette=None, gt_undistort=False):
        """`add_view` for a batch: up to eight views share their rasteriser launches.  Ground-truth images that share dtype, strides
        and memory go to the library as one batch; a mixed list is scored view by view.  `gt_resize`, `gt_map`, `gt_palette`: see
        add_image.  `gt_undistort=True`: the ground truth of every `data.LensCamera` is on that lens's sensor grid, at any size; it is
        undistorted on the device first, sampled nearest, and the pixels where the view looks past the sensor are ignored.  Not
        together with `gt_resize=`."""
        cameras, gt_images = list(cameras), list(gt_images)
        n = len(cameras)
        if len(gt_images) != n:
            raise ValueError("add_views needs one ground-truth image per camera")
        if gt_undistort:
            if gt_resize is not None:
                raise ValueError("add_views: gt_undistort=True cannot be combined with gt_resize= (the sensor image is undistorted at any size)")
            done = [self._undistorted_gt(gt_images[i], cam, gt_map, gt_palette, "ground truth %d" % i) for i, cam in enumerate(cameras)]
            gt_images = [d[0] if d[1] is None and d[2] is None else self._prepared_gt(d[0], tuple(cam.resolution), None, d[1], "ground truth %d" % i, d[2])
                         for i, (d, cam) in enumerate(zip(done, cameras))]
            gt_map = gt_palette = None
        if gt_resize is not None or gt_map is not None or gt_palette is not None:
            gt_images = [self._prepared_gt(gt_images[i], tuple(cam.resolution), gt_resize, gt_map, "ground truth %d" % i, gt_palette)
                         for i, cam in enumerate(cameras)]
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

    def add_probs(self, probs, gt, dont_care_threshold=None, probs_dtype=None, labels_out=False, resize=None, gt_map=None, gt_palette=None):
        """Score a class-vector image itself -- the network's own prediction, the baseline the fused mesh is compared with: `probs`
        (W,H,C) with C = classes (what `MeshAggregator.add` takes), arg-maxed by the rule of `argmax_labels_device` and counted against
        `gt` integer (W,H) in the same pass.  With `dont_care_threshold` a pixel whose class sum is below it counts as don't care.
        `labels_out=True` returns the label image of that pass as a (W,H) `DeviceArray`.  With `resize="bilinear"` a `probs` image
        whose (w,h) is not `gt`'s (W,H) is scored as `resize_probs(probs, (W,H))` would be (resize.py), without that image being
        built; with `resize=None` such a pair is refused.  `gt_map`: ground-truth value v counts as map[v] (see add_image; the ground
        truth defines the target size, so there is nothing to resample on its side); `gt_palette`: a colour image as ground truth (see
        add_image)."""
        from .resize import resize_mode
        mode = resize_mode(resize)
        gt = self._prepared_gt(gt, None, None, gt_map, "ground truth", gt_palette)
        streams = []
        thr = _threshold(dont_care_threshold)
        pp, pmem, (W, H, C), code, pstr, k0 = _describe_probs(probs, probs_dtype, self.device, streams)
        if C != self.classes:
            raise ValueError("probs image has %d classes, the confusion matrix was built for %d" % (C, self.classes))
        gshape = tuple(getattr(gt, "shape", None) or np.shape(gt)) if mode is not None else (W, H)
        if mode is not None and len(gshape) == 2 and gshape != (W, H):
            return self._add_probs_resized(streams, thr, (pp, pmem, (W, H, C), code, pstr, k0), gt, gshape, labels_out, mode)
        gp, gmem, gcode, gstr, k1 = self._gt(gt, 2, (W, H), "ground truth", streams)
        out, optr, ocode, ostr, dc = None, None, 0, None, 0
        if labels_out:
            dt, dc = _label_out(C, None if C <= 65535 else np.int32, None)
            out = _label_image_like(W, H, pstr, dt, self.device)
            optr, ocode, ostr = ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], _c64(out.strides)
        if W and H:
            _lib.check(_lib.lib().smesh_confusion_add_probs(self._h, ctypes.c_void_p(pp), code, _c64(pstr), pmem,
                                                            ctypes.c_void_p(gp), gcode, _c64(gstr), gmem, W, H, thr, optr, ocode, ostr, dc))
        self._done(streams, [k0, k1])
        return out

    def _add_probs_resized(self, streams, thr, desc, gt, gshape, labels_out, mode):
        """`add_probs` for a (w,h,C) image against (W,H) ground truth: `smesh_confusion_add_probs_resized`."""
        pp, pmem, (w, h, C), code, pstr, k0 = desc
        W, H = int(gshape[0]), int(gshape[1])
        if W and H and not (w and h):
            raise ValueError("an empty probs image %s cannot be resampled to %s" % ((w, h), (W, H)))
        gp, gmem, gcode, gstr, k1 = self._gt(gt, 2, (W, H), "ground truth", streams)
        out, optr, ocode, ostr, dc = None, None, 0, None, 0
        if labels_out:
            dt, dc = _label_out(C, None if C <= 65535 else np.int32, None)
            out = DeviceBuffer(max(W * H * dt.itemsize, 1), self.device).view((W, H), dt)
            optr, ocode, ostr = ctypes.c_void_p(out.ptr), _lib.LBL_CODES[dt.name], _c64(out.strides)
        if W and H:
            _lib.check(_lib.lib().smesh_confusion_add_probs_resized(self._h, ctypes.c_void_p(pp), code, _c64(pstr), pmem, w, h,
                                                                    ctypes.c_void_p(gp), gcode, _c64(gstr), gmem, W, H, thr, mode,
                                                                    optr, ocode, ostr, dc))
        self._done(streams, [k0, k1])
        return out

    def add_probs_many(self, probs_images, gt_images, dont_care_threshold=None, probs_dtype=None, labels_out=False, resize=None, gt_map=None,
                       gt_palette=None):
        """`add_probs` for a batch: a loop.  Returns the list of label images with `labels_out=True`."""
        probs_images, gt_images = list(probs_images), list(gt_images)
        if len(probs_images) != len(gt_images):
            raise ValueError("add_probs_many needs one ground-truth image per class-vector image")
        outs = [self.add_probs(p, g, dont_care_threshold, probs_dtype, labels_out, resize, gt_map, gt_palette) for p, g in zip(probs_images, gt_images)]
        return outs if labels_out else None

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
