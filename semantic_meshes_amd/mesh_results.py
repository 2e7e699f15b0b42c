"""Results on the fused mesh beyond its faces (include/smesh_vertices.h, smesh_points.h, smesh_face_graph.h, smesh_face_segments.h,
smesh_segment_stats.h): VertexTransfer, SurfaceIndex, PointTransfer, FaceGraph and FaceSegments, and the plumbing they share -- a library handle that is
destroyed with its owner, the faces check, a `source` of face rows resolved once, and a fresh result on the host or in HBM.
`fusion` re-exports the classes; that is where callers find them."""
import ctypes
import math

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, describe, release_to, result_empty
from .fusion import _MeshAggregator


class _Handle:
    """Owns a library handle `_h`; `_destroy` names the library function that gives it back."""
    _h = None
    _destroy = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                getattr(_lib.lib(), self._destroy)(h)
            except Exception:
                pass


def _check_faces(faces, num_vertices):
    """`faces` as a contiguous int32 [F,3] array whose indices lie in [0, int(num_vertices))."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError("faces must be an integer array [F,3], got %s %s" % (f.dtype, f.shape))
    num_vertices = int(num_vertices)
    if num_vertices < 0:
        raise ValueError("num_vertices must be >= 0")
    if f.size and (f.min() < 0 or f.max() >= num_vertices):      # (the library checks again, on the device)
        raise ValueError("face indices out of range [0, %d)" % num_vertices)
    return np.ascontiguousarray(f, dtype=np.int32)


def _texel_layout_faces(texel_renderer):
    """For `from_renderer`: the faces of a texel renderer's layout, the order `face_annotations()` returns its rows in."""
    if not hasattr(texel_renderer, "texel_layout"):
        raise ValueError("from_renderer needs a texel renderer (render.texels)")
    return texel_renderer.texel_layout()[0]


def _out(shape, dtype, device, on_device):
    """(array, pointer, memkind) of a fresh result."""
    n = math.prod(shape) * np.dtype(dtype).itemsize      # (not np.prod: microseconds that a short gather's caller would see)
    if on_device:
        out = DeviceBuffer(max(n, 4), device).view(shape, dtype)
        return out, ctypes.c_void_p(out.ptr), _lib.MEM_DEVICE
    out = result_empty(shape, dtype) if len(shape) == 2 else np.empty(shape, dtype)
    return out, out.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST


def _rows_and_labels(n, C, device, want_rows, want_labels, on_device):
    """(rows [n,C] or None, labels [n] or None, the three arguments the library takes for them)."""
    rows = labels = prow = plab = None
    if want_rows:
        rows, prow, _ = _out((n, C), np.float32, device, on_device)
    if want_labels:
        labels, plab, _ = _out((n,), np.int32, device, on_device)
    return rows, labels, (prow, plab, _lib.MEM_DEVICE if on_device else _lib.MEM_HOST)


class _Source:
    """A `source` of face rows resolved for an owner on `device` that has `rows` faces: a MeshAggregator (`is_aggregator`; the caller
    hands `source._h` to the library), or a float32 [rows,C] array on the host or the device as `ptr`, `memkind`.  `classes` is C.
    `mesh` and `owner` are the nouns of the error texts.  `finish()` after the library call: it drains an aggregator and
    always releases `streams` -- the producers of a device array, and whatever the caller collected in the list it passed in."""

    def __init__(self, source, rows, device, mesh, owner, streams=None):
        self.source, self.device, self.streams = source, device, [] if streams is None else streams
        self.is_aggregator = isinstance(source, _MeshAggregator)
        if self.is_aggregator:
            if source.primitives != rows:
                raise ValueError("the aggregator has %d primitives, %s %d faces" % (source.primitives, mesh, rows))
            if source.device != device:
                raise ValueError("aggregator and %s live on different devices" % owner)
            self.classes = source.classes
        else:
            _same_device(source, device, "face rows")
            ptr, self.memkind, self.classes, self._keep = _dense_rows(source, rows, "face rows", device, self.streams)
            self.ptr = ctypes.c_void_p(ptr)

    def finish(self):
        if self.is_aggregator:
            self.source._drain()
        release_to(self.device, self.streams)


def _same_device(obj, device, what):
    if isinstance(obj, DeviceArray) and obj.device != device:
        raise ValueError("%s lives on device %d, not on device %d" % (what, obj.device, device))


def _dense_rows(source, rows, what, device, streams):
    """(pointer, memkind, C, keep-alive) of a dense float32 [rows, C] array on the host or the device, C >= 1."""
    if isinstance(source, np.ndarray) and source.dtype != np.float32:
        raise ValueError("%s must be float32, got %s" % (what, source.dtype))
    ptr, mem, shape, dt, strides, keep = describe(source, 2, what, device, streams)
    if dt != np.float32:
        raise ValueError("%s must be float32, got %s" % (what, dt))
    if shape[0] != rows or shape[1] < 1:
        raise ValueError("%s must be float32[%d,C], got shape %s" % (what, rows, tuple(shape)))
    if shape[0] > 1 and tuple(strides) != (shape[1], 1) or shape[1] > 1 and strides[1] != 1:
        if mem != _lib.MEM_HOST:
            raise ValueError("%s must be dense (row-major, no padding)" % what)
        keep = np.ascontiguousarray(keep)
        ptr = keep.ctypes.data
    return ptr, mem, int(shape[1]), keep


def _dense_vector(values, n, what, per, device, streams):
    """(pointer or None, memkind, keep-alive) of an optional float32 vector of `n` elements (`per`: what it has one element of), dense,
    on the host or on `device`."""
    if values is None:
        return None, _lib.MEM_HOST, None
    if isinstance(values, np.ndarray) and values.dtype != np.float32:
        raise ValueError("%s must be float32, got %s" % (what, values.dtype))
    _same_device(values, device, what)
    ptr, mem, shape, dt, strides, keep = describe(values, 1, what, device, streams)
    if dt != np.float32:
        raise ValueError("%s must be float32, got %s" % (what, dt))
    if shape[0] != n:
        raise ValueError("%s must have %s (%d), got %d" % (what, per, n, shape[0]))
    if shape[0] > 1 and strides[0] != 1:
        if mem != _lib.MEM_HOST:
            raise ValueError("%s must be dense" % what)
        keep = np.ascontiguousarray(keep)
        ptr = keep.ctypes.data
    return ctypes.c_void_p(ptr), mem, keep


class VertexTransfer(_Handle):
    """Face annotations to per-vertex annotations and labels, on the device (include/smesh_vertices.h) -- what the reference's
    evaluation does on the host with a Python loop over every face, `tf.gather`, `reduce_sum`, a 0.9 "don't care" threshold and a
    renormalisation (eval-scannet/eval_scannet.py:249-287).

    `faces`: int[F,3], `num_vertices`: V.  The vertex-to-faces table is built once, on `device`.  A `source` is a MeshAggregator
    over the F faces (its `get()` never leaves the device), a float32 [F,C] numpy array, or a dense float32 [F,C] device array.
    For vertex v, sums[v] is the float32 sum of the rows of v's faces in ascending face order; annotations[v] is sums[v] divided by
    its total, or all zero where that total is below `dont_care_threshold`; labels[v] is the argmax of sums[v], -1 where don't care."""

    _destroy = "smesh_vertex_map_destroy"

    def __init__(self, faces, num_vertices, device=0):
        f = _check_faces(faces, num_vertices)
        self.num_vertices, self.num_faces, self.device = int(num_vertices), len(f), int(device)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_vertex_map_create(f.ctypes.data_as(ctypes.c_void_p), len(f), self.num_vertices, self.device,
                                                     ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_mesh(cls, mesh, device=0):
        return cls(mesh.faces, len(mesh.vertices), device)

    @classmethod
    def from_renderer(cls, texel_renderer, num_vertices):
        """For a texel renderer: its layout's faces, the order `face_annotations()` returns its rows in."""
        return cls(_texel_layout_faces(texel_renderer), num_vertices, texel_renderer.device)

    def adjacency(self):
        """The vertex-to-faces table as `(offsets uint64[V+1], faces uint32[nnz])`: the faces of vertex v, ascending, are
        `faces[offsets[v]:offsets[v+1]]`."""
        nnz = ctypes.c_uint64()
        _lib.check(_lib.lib().smesh_vertex_map_size(self._h, None, None, ctypes.byref(nnz)))
        offsets, faces = np.empty(self.num_vertices + 1, np.uint64), np.empty(int(nnz.value), np.uint32)
        _lib.check(_lib.lib().smesh_vertex_map_adjacency(self._h, offsets.ctypes.data_as(ctypes.c_void_p), faces.ctypes.data_as(ctypes.c_void_p)))
        return offsets, faces

    def _run(self, source, mode, threshold, want_rows, want_labels, on_device):
        src = _Source(source, self.num_faces, self.device, "the mesh", "VertexTransfer")
        rows, labels, outs = _rows_and_labels(self.num_vertices, src.classes, self.device, want_rows, want_labels, on_device)
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_vertex_annotations(source._h, self._h, mode, float(threshold), *outs))
        else:
            _lib.check(_lib.lib().smesh_vertex_map_gather(self._h, src.ptr, src.memkind, src.classes, mode, float(threshold), *outs))
        src.finish()
        return rows, labels

    def sums(self, source):
        """float32 [V,C]: per vertex, the sum of its faces' rows."""
        return self._run(source, _lib.VTX_SUMS, 0.0, True, False, False)[0]

    def annotations(self, source, dont_care_threshold=0.9):
        """float32 [V,C]: the sums renormalised; all-zero rows where the sum is below `dont_care_threshold` (eval_scannet.py:271-287)."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, False)[0]

    def labels(self, source, dont_care_threshold=0.9):
        """int32 [V]: the class with the largest sum (the lowest one among equals), -1 where don't care.  No [V,C] array is made."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, False)[1]

    def annotations_device(self, source, dont_care_threshold=0.9):
        """`annotations()` left in HBM: a `DeviceArray` in a fresh allocation owned by the returned object."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, True)[0]

    def labels_device(self, source, dont_care_threshold=0.9):
        """`labels()` left in HBM."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, True)[1]


def _dense_points(points, device, streams):
    """(pointer, memkind, N, keep-alive) of a dense float32 [N,3] array of query points on the host or the device."""
    if isinstance(points, np.ndarray) and points.dtype != np.float32:
        raise ValueError("points must be float32, got %s" % points.dtype)
    _same_device(points, device, "points")
    ptr, mem, shape, dt, strides, keep = describe(points, 2, "points", device, streams)
    if dt != np.float32:
        raise ValueError("points must be float32, got %s" % dt)
    if shape[1] != 3:
        raise ValueError("points must be float32[N,3], got shape %s" % (tuple(shape),))
    if shape[0] > 1 and tuple(strides) != (3, 1) or strides[1] != 1:
        if mem != _lib.MEM_HOST:
            raise ValueError("points must be dense (row-major, no padding)")
        keep = np.ascontiguousarray(keep)
        ptr = keep.ctypes.data
    return ptr, mem, int(shape[0]), keep


class SurfaceIndex(_Handle):
    """The closest face of arbitrary points, on the device (include/smesh_points.h): a uniform grid over the faces of a mesh, built
    once on `device`.  `vertices`: float32 [V,3], `faces`: int [F,3].  The closest face of a point is defined to the bit -- the
    smallest float32 `dist2` of the header's rule over ALL faces, the lowest face among equal values -- and the grid only finds
    it faster."""

    _destroy = "smesh_surface_index_destroy"

    def __init__(self, vertices, faces, device=0):
        v = np.asarray(vertices)
        if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind != "f":
            raise ValueError("vertices must be a float array [V,3], got %s %s" % (v.dtype, v.shape))
        v, f = np.ascontiguousarray(v, dtype=np.float32), _check_faces(faces, len(v))
        self.num_faces, self.device = len(f), int(device)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_surface_index_create(v.ctypes.data_as(ctypes.c_void_p), len(v), f.ctypes.data_as(ctypes.c_void_p),
                                                        len(f), self.device, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_mesh(cls, mesh, device=0):
        return cls(mesh.vertices, mesh.faces, device)

    @classmethod
    def from_renderer(cls, texel_renderer, vertices):
        """For a texel renderer: its layout's faces, the order `face_annotations()` returns its rows in."""
        return cls(vertices, _texel_layout_faces(texel_renderer), texel_renderer.device)

    def stats(self):
        """`dict(faces, dims, entries, large_faces)`: the grid's dimensions, the entries of its cells' face lists, and the faces
        that every query tests (a box over too many cells, or no area)."""
        F, entries, large = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        dims = (ctypes.c_uint32 * 3)()
        _lib.check(_lib.lib().smesh_surface_index_stats(self._h, ctypes.byref(F), dims, ctypes.byref(entries), ctypes.byref(large)))
        return dict(faces=int(F.value), dims=tuple(int(d) for d in dims), entries=int(entries.value), large_faces=int(large.value))

    def _nearest(self, points, max_distance, on_device):
        R = float("inf") if max_distance is None else float(max_distance)
        if not R >= 0:
            raise ValueError("max_distance must be >= 0 (or None), got %r" % (max_distance,))
        streams = []
        ptr, mem, N, keep = _dense_points(points, self.device, streams)
        faces, pf, omem = _out((N,), np.int32, self.device, on_device)
        dist2, pd, omem = _out((N,), np.float32, self.device, on_device)
        _lib.check(_lib.lib().smesh_surface_index_nearest(self._h, ctypes.c_void_p(ptr), N, mem, R, pf, pd, omem))
        release_to(self.device, streams)
        return faces, dist2

    def nearest(self, points, max_distance=None):
        """`(faces int32 [N], dist2 float32 [N])` of float32 [N,3] `points` (numpy, or a dense device array): the closest face and
        its squared distance; `(-1, inf)` for a point farther than `max_distance` from every face, a point with a non-finite
        coordinate, and every point of a mesh without faces."""
        return self._nearest(points, max_distance, False)

    def nearest_device(self, points, max_distance=None):
        """`nearest()` left in HBM: two `DeviceArray`s."""
        return self._nearest(points, max_distance, True)


class PointTransfer:
    """Fused results for points that are not the mesh's vertices: the ground truth's vertices on a simplified, COLMAP or texel mesh, a
    lidar scan, a submission file.  Holds the closest face of every point (`SurfaceIndex.nearest_device`) on the device; a `source` is
    what it is for `VertexTransfer` -- a MeshAggregator over the index's F faces (its `get()` never leaves the device), a float32
    [F,C] numpy array or a dense float32 [F,C] device array; for a texel renderer, `renderer.face_annotations(aggregator)`.
    sums[i] is the row of point i's face (zeros without one); annotations[i] is that row divided by its total, all zero where the
    total is below `dont_care_threshold` or the point has no face; labels[i] is the row's argmax, -1 where don't care."""

    def __init__(self, index, points, max_distance=None):
        if not isinstance(index, SurfaceIndex):
            raise ValueError("PointTransfer needs a SurfaceIndex")
        self.index, self.device = index, index.device
        self.faces, self.dist2 = index.nearest_device(points, max_distance)
        self.num_points = self.faces.shape[0]

    def _run(self, source, mode, threshold, want_rows, want_labels, on_device):
        N, F = self.num_points, self.index.num_faces
        src = _Source(source, F, self.device, "the indexed mesh", "PointTransfer")
        rows, labels, outs = _rows_and_labels(N, src.classes, self.device, want_rows, want_labels, on_device)
        pf = ctypes.c_void_p(self.faces.ptr)
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_point_annotations(source._h, pf, N, _lib.MEM_DEVICE, mode, float(threshold), *outs))
        else:
            _lib.check(_lib.lib().smesh_point_gather(src.ptr, src.memkind, F, src.classes, pf, N, _lib.MEM_DEVICE, mode, float(threshold),
                                                    *outs))
        src.finish()
        return rows, labels

    def sums(self, source):
        """float32 [N,C]: per point, the row of its closest face."""
        return self._run(source, _lib.VTX_SUMS, 0.0, True, False, False)[0]

    def annotations(self, source, dont_care_threshold=0.9):
        """float32 [N,C]: the rows renormalised; all-zero rows where the total is below `dont_care_threshold` or there is no face."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, False)[0]

    def labels(self, source, dont_care_threshold=0.9):
        """int32 [N]: the class with the largest value (the lowest one among equals), -1 where don't care.  No [N,C] array is made."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, False)[1]

    def sums_device(self, source):
        """`sums()` left in HBM: a `DeviceArray` in a fresh allocation owned by the returned object."""
        return self._run(source, _lib.VTX_SUMS, 0.0, True, False, True)[0]

    def annotations_device(self, source, dont_care_threshold=0.9):
        """`annotations()` left in HBM."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, True)[0]

    def labels_device(self, source, dont_care_threshold=0.9):
        """`labels()` left in HBM: what `ConfusionMatrix.add` takes beside the points' ground truth."""
        return self._run(source, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, True)[1]


class FaceGraph(_Handle):
    """Fused rows propagated along the surface, on the device (include/smesh_face_graph.h): for every face the faces across its
    edges, built once on `device`, and T averaging iterations over them.  The reference has no such step.

    `faces`: int[F,3], `num_vertices`: V.  A `source` is what it is for `VertexTransfer`: a MeshAggregator over the F faces (its
    `get()` never leaves the device), a float32 [F,C] numpy array, or a dense float32 [F,C] device array.  In every iteration a face
    takes the mean m of its INFORMED neighbours (those whose row total is > 0; weighted by `weights`, one float32 per entry of
    `adjacency()`, e.g. `normal_weights()`).  `smooth*`: x <- (1 - alpha) x0 + alpha m.  `fill*`: a face whose own total reaches
    `observed_threshold` keeps its row, every other face takes m, so the front advances one ring of faces per iteration.  The
    result is finished as `VertexTransfer` finishes a vertex row: `*_sums` the rows as they are, the plain form divided by their
    total (all zero below `dont_care_threshold`), `*_labels` their argmax (-1 where don't care); `*_device` leaves it in HBM.
    `return_unreached=True`: `(result, number of faces whose final total is not > 0)`."""

    _destroy = "smesh_face_graph_destroy"

    def __init__(self, faces, num_vertices, device=0):
        self._faces = _check_faces(faces, num_vertices)             # (normal_weights reads them again)
        self.num_vertices, self.num_faces, self.device = int(num_vertices), len(self._faces), int(device)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().smesh_face_graph_create(self._faces.ctypes.data_as(ctypes.c_void_p), self.num_faces, self.num_vertices,
                                                     self.device, ctypes.byref(h)))
        self._h = h
        nnz = ctypes.c_uint64()
        _lib.check(_lib.lib().smesh_face_graph_size(self._h, None, None, ctypes.byref(nnz)))
        self.num_entries = int(nnz.value)

    @classmethod
    def from_mesh(cls, mesh, device=0):
        return cls(mesh.faces, len(mesh.vertices), device)

    @classmethod
    def from_renderer(cls, texel_renderer, num_vertices):
        """For a texel renderer: its layout's faces, the order `face_annotations()` returns its rows in."""
        return cls(_texel_layout_faces(texel_renderer), num_vertices, texel_renderer.device)

    def adjacency(self):
        """The graph as `(offsets uint64[F+1], neighbours uint32[nnz])`: the faces across the edges of face f, edge slot after edge
        slot and ascending within a slot, are `neighbours[offsets[f]:offsets[f+1]]`."""
        offsets, nbr = np.empty(self.num_faces + 1, np.uint64), np.empty(self.num_entries, np.uint32)
        _lib.check(_lib.lib().smesh_face_graph_adjacency(self._h, offsets.ctypes.data_as(ctypes.c_void_p), nbr.ctypes.data_as(ctypes.c_void_p)))
        return offsets, nbr

    # ---- normal-agreement weights ------------------------------------------------------------------------------------------------
    def _normal_weights(self, vertices, power, two_sided, on_device):
        if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 1 <= int(power) <= _lib.FG_MAX_POWER:
            raise ValueError("power must be an int in 1 .. %d, got %r" % (_lib.FG_MAX_POWER, power))
        streams = []
        ptr, mem, N, keep = _dense_points(vertices, self.device, streams)
        if N != self.num_vertices:
            raise ValueError("vertices must be float32[%d,3], got %d rows" % (self.num_vertices, N))
        out, pout, omem = _out((self.num_entries,), np.float32, self.device, on_device)
        _lib.check(_lib.lib().smesh_face_graph_normal_weights(self._h, self._faces.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), mem,
                                                             int(power), 1 if two_sided else 0, pout, omem))
        release_to(self.device, streams)
        return out

    def normal_weights(self, vertices, power=4, two_sided=True):
        """One float32 weight per entry of `adjacency()`, a `DeviceArray`: the cosine between the two faces' normals (its absolute
        value with `two_sided`), clamped to [0, 1] and raised to `power` -- 1 across a flat edge, 0 across a right angle or next to
        a face without area.  `vertices`: float32 [V,3], numpy or a dense device array."""
        return self._normal_weights(vertices, power, two_sided, True)

    def normal_weights_host(self, vertices, power=4, two_sided=True):
        """`normal_weights()` as a numpy array."""
        return self._normal_weights(vertices, power, two_sided, False)

    def _entry_weights(self, weights, streams):
        """(pointer or None, memkind, keep-alive) of per-entry weights: float32, `num_entries` elements, dense, on this device."""
        return _dense_vector(weights, self.num_entries, "weights", "one element per entry of the graph", self.device, streams)

    # ---- face areas --------------------------------------------------------------------------------------------------------------
    def _face_areas(self, vertices, on_device):
        streams = []
        ptr, mem, N, keep = _dense_points(vertices, self.device, streams)
        if N != self.num_vertices:
            raise ValueError("vertices must be float32[%d,3], got %d rows" % (self.num_vertices, N))
        out, pout, omem = _out((self.num_faces,), np.float32, self.device, on_device)
        _lib.check(_lib.lib().smesh_segment_stats_face_areas(self._h, self._faces.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), mem,
                                                            pout, omem))
        release_to(self.device, streams)
        return out

    def face_areas(self, vertices):
        """float32 [F]: the area of every face (include/smesh_segment_stats.h), half the length of the normal that `normal_weights()`
        uses; +0 for a face without area.  `vertices`: float32 [V,3], numpy or a dense device array."""
        return self._face_areas(vertices, False)

    def face_areas_device(self, vertices):
        """`face_areas()` left in HBM: what `FaceSegments.areas*` and `pool*(face_weights=...)` take."""
        return self._face_areas(vertices, True)

    # ---- propagation -------------------------------------------------------------------------------------------------------------
    def _run(self, source, fg_mode, iterations, alpha, observed_threshold, weights, out_mode, threshold, want_rows, want_labels, on_device,
             return_unreached):
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0 or iterations > 0xFFFFFFFF:
            raise ValueError("iterations must be a non-negative int, got %r" % (iterations,))
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("alpha must lie in [0, 1], got %r" % (alpha,))
        streams = []
        pw, wmem, wkeep = self._entry_weights(weights, streams)
        src = _Source(source, self.num_faces, self.device, "the mesh", "FaceGraph", streams)
        rows, labels, (prow, plab, omem) = _rows_and_labels(self.num_faces, src.classes, self.device, want_rows, want_labels, on_device)
        unreached = ctypes.c_uint64(0)
        tail = (pw, wmem, fg_mode, int(iterations), float(alpha), float(observed_threshold), out_mode, float(threshold), prow, plab,
                ctypes.byref(unreached) if return_unreached else None, omem)
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_face_propagate(source._h, self._h, *tail))
        else:
            _lib.check(_lib.lib().smesh_face_graph_propagate(self._h, src.ptr, src.memkind, src.classes, *tail))
        src.finish()
        result = rows if want_rows else labels
        return (result, int(unreached.value)) if return_unreached else result

    def _smooth(self, source, iterations, alpha, weights, out_mode, threshold, want_labels, on_device, return_unreached):
        return self._run(source, _lib.FG_SMOOTH, iterations, alpha, 0.0, weights, out_mode, threshold, not want_labels, want_labels,
                         on_device, return_unreached)

    def _fill(self, source, iterations, observed_threshold, weights, out_mode, threshold, want_labels, on_device, return_unreached):
        return self._run(source, _lib.FG_FILL, iterations, 0.0, observed_threshold, weights, out_mode, threshold, not want_labels,
                         want_labels, on_device, return_unreached)

    def smooth(self, source, iterations=10, alpha=0.5, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """float32 [F,C]: the smoothed rows renormalised; all-zero rows where their total is below `dont_care_threshold`."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, False, return_unreached)

    def smooth_sums(self, source, iterations=10, alpha=0.5, weights=None, return_unreached=False):
        """float32 [F,C]: the smoothed rows as they are."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_SUMS, 0.0, False, False, return_unreached)

    def smooth_labels(self, source, iterations=10, alpha=0.5, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """int32 [F]: the class with the largest smoothed value (the lowest one among equals), -1 where don't care."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, return_unreached)

    def smooth_device(self, source, iterations=10, alpha=0.5, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """`smooth()` left in HBM: a `DeviceArray` in a fresh allocation owned by the returned object."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, return_unreached)

    def smooth_sums_device(self, source, iterations=10, alpha=0.5, weights=None, return_unreached=False):
        """`smooth_sums()` left in HBM."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_SUMS, 0.0, False, True, return_unreached)

    def smooth_labels_device(self, source, iterations=10, alpha=0.5, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """`smooth_labels()` left in HBM: a label table for `LabelRenderer`, `ConfusionMatrix.add_views` and `PointTransfer`."""
        return self._smooth(source, iterations, alpha, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, True, return_unreached)

    def fill(self, source, iterations=32, observed_threshold=0.9, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """float32 [F,C]: observed faces as they were, the others filled from them, renormalised; all-zero rows where the total is
        below `dont_care_threshold` (a face the front has not reached)."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, False,
                          return_unreached)

    def fill_sums(self, source, iterations=32, observed_threshold=0.9, weights=None, return_unreached=False):
        """float32 [F,C]: the filled rows as they are."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_SUMS, 0.0, False, False, return_unreached)

    def fill_labels(self, source, iterations=32, observed_threshold=0.9, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """int32 [F]: the class with the largest filled value (the lowest one among equals), -1 where don't care."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False,
                          return_unreached)

    def fill_device(self, source, iterations=32, observed_threshold=0.9, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """`fill()` left in HBM."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True,
                          return_unreached)

    def fill_sums_device(self, source, iterations=32, observed_threshold=0.9, weights=None, return_unreached=False):
        """`fill_sums()` left in HBM."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_SUMS, 0.0, False, True, return_unreached)

    def fill_labels_device(self, source, iterations=32, observed_threshold=0.9, weights=None, dont_care_threshold=0.9, return_unreached=False):
        """`fill_labels()` left in HBM."""
        return self._fill(source, iterations, observed_threshold, weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, True,
                          return_unreached)

    # ---- segments ----------------------------------------------------------------------------------------------------------------
    def segments(self, source, weights=None, min_weight=None, dont_care_threshold=0.9):
        """The connected components of equal labels over the graph, a `FaceSegments` (include/smesh_face_segments.h).

        `source`: labels as a 1-D integer array [F] (numpy, or an int32 device array such as `labels_device()` returns; a negative
        label is "don't care" and belongs to no segment), or what every other method takes -- an aggregator or float32 [F,C] rows,
        whose labels are their argmax, -1 below `dont_care_threshold`.  With `weights` (one float32 per entry of `adjacency()`) an
        entry links its two faces only where its weight is >= `min_weight`, which then has to be given: there is no default.  One
        passing entry in either face's list links the two."""
        if (weights is None) != (min_weight is None):
            raise ValueError("min_weight is required with weights and only with weights")
        if min_weight is not None and (isinstance(min_weight, bool) or not isinstance(min_weight, (int, float, np.integer, np.floating))):
            raise ValueError("min_weight must be a number, got %r" % (min_weight,))
        F = self.num_faces
        streams = []
        pw, wmem, wkeep = self._entry_weights(weights, streams)
        mw = 0.0 if min_weight is None else float(min_weight)
        h = ctypes.c_void_p()
        if isinstance(source, _MeshAggregator):
            src = _Source(source, F, self.device, "the mesh", "FaceGraph", streams)
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_face_segments(source._h, self._h, float(dont_care_threshold), pw, wmem, mw, ctypes.byref(h)))
            src.finish()
        else:
            shape = source.shape if hasattr(source, "shape") else np.shape(source)
            if len(shape) == 2:      # rows: their labels by the finishing step (T = 0), left on the device
                source = self.smooth_labels_device(source, 0, dont_care_threshold=dont_care_threshold)
            if isinstance(source, np.ndarray) or not hasattr(source, "shape"):
                a = np.asarray(source)
                if a.ndim != 1 or a.dtype.kind not in "iu" or len(a) != F:
                    raise ValueError("labels must be an integer array [%d], got %s %s" % (F, a.dtype, a.shape))
                if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
                    raise ValueError("labels must fit int32")
                source = np.ascontiguousarray(a, dtype=np.int32)
            _same_device(source, self.device, "labels")
            ptr, mem, lshape, ldt, lstrides, keep = describe(source, 1, "labels", self.device, streams)
            if ldt != np.int32 or lshape[0] != F:
                raise ValueError("labels must be int32[%d], got %s %s" % (F, ldt, tuple(lshape)))
            if lshape[0] > 1 and lstrides[0] != 1:
                raise ValueError("labels must be dense")
            _lib.check(_lib.lib().smesh_face_segments_create(self._h, ctypes.c_void_p(ptr), mem, pw, wmem, mw, ctypes.byref(h)))
            release_to(self.device, streams)
        return FaceSegments(h, self.device)


def _min_faces(min_faces):
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)) or min_faces < 0 or min_faces > 0xFFFFFFFF:
        raise ValueError("min_faces must be a non-negative int, got %r" % (min_faces,))
    return int(min_faces)


class FaceSegments(_Handle):
    """The segments of a labelled mesh, on the device (include/smesh_face_segments.h); made by `FaceGraph.segments()`.

    A segment is a connected component of faces with one label (>= 0) under the graph's links; segments are numbered 0 .. count-1
    in the order of their lowest face.  `ids()`: int32 [F], the segment of every face, -1 for an unlabelled one.  Per segment:
    `first_faces()` uint32, `labels()` int32, `sizes()` uint32 (faces).  The `*_device()` forms leave a `DeviceArray` in HBM.
    `despeckle_*(min_faces)`: a face is kept when its segment has at least `min_faces` faces; `despeckle_labels*` gives the labels
    with every other face at -1 (a label table like any other, for `LabelRenderer`, `ConfusionMatrix.add*`, `PointTransfer`);
    `despeckle_sums*` gives the rows of `source` with the rows of removed faces zeroed, a source for `FaceGraph.fill_*`, which
    lets the surroundings grow back in.  Everything is an integer result: two calls agree in every bit.
    `members()`, `pool*`, `pooled_face_*`, `areas()` and `despeckle_*_by(measure, minimum)` (include/smesh_segment_stats.h) add up
    what the faces of a segment carry, in a stated order, so these float results agree in every bit too."""

    _destroy = "smesh_face_segments_destroy"

    def __init__(self, handle, device):
        self._h, self.device = handle, int(device)
        F, S, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(_lib.lib().smesh_face_segments_size(self._h, ctypes.byref(F), ctypes.byref(S), ctypes.byref(n)))
        self.num_faces, self.count, self.num_labelled = int(F.value), int(S.value), int(n.value)

    def _get(self, which, on_device):
        shape, dtype = [((self.num_faces,), np.int32), ((self.count,), np.uint32), ((self.count,), np.int32), ((self.count,), np.uint32)][which]
        out, ptr, mem = _out(shape, dtype, self.device, on_device)
        args = [None] * 4
        args[which] = ptr
        _lib.check(_lib.lib().smesh_face_segments_get(self._h, *args, mem))
        return out

    def ids(self):
        """int32 [F]: the segment of every face, -1 for an unlabelled face."""
        return self._get(0, False)

    def first_faces(self):
        """uint32 [count]: the lowest face of every segment (ascending)."""
        return self._get(1, False)

    def labels(self):
        """int32 [count]: the label of every segment."""
        return self._get(2, False)

    def sizes(self):
        """uint32 [count]: the number of faces of every segment."""
        return self._get(3, False)

    def ids_device(self):
        return self._get(0, True)

    def first_faces_device(self):
        return self._get(1, True)

    def labels_device(self):
        return self._get(2, True)

    def sizes_device(self):
        return self._get(3, True)

    def _despeckle_labels(self, min_faces, return_removed, on_device):
        min_faces = _min_faces(min_faces)
        out, ptr, mem = _out((self.num_faces,), np.int32, self.device, on_device)
        faces, segs = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(_lib.lib().smesh_face_segments_despeckle_labels(self._h, min_faces, ptr, mem, ctypes.byref(faces) if return_removed else None,
                                                                  ctypes.byref(segs) if return_removed else None))
        return (out, int(faces.value), int(segs.value)) if return_removed else out

    def despeckle_labels(self, min_faces, return_removed=False):
        """int32 [F]: the label of every kept face, -1 elsewhere.  `return_removed=True`: `(labels, removed faces, removed segments)`."""
        return self._despeckle_labels(min_faces, return_removed, False)

    def despeckle_labels_device(self, min_faces, return_removed=False):
        """`despeckle_labels()` left in HBM."""
        return self._despeckle_labels(min_faces, return_removed, True)

    def _despeckle_sums(self, source, min_faces, on_device):
        min_faces = _min_faces(min_faces)
        src = _Source(source, self.num_faces, self.device, "the segments", "FaceSegments")
        out, ptr, mem = _out((self.num_faces, src.classes), np.float32, self.device, on_device)
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_face_segments_despeckle(source._h, self._h, min_faces, ptr, mem))
        else:
            _lib.check(_lib.lib().smesh_face_segments_despeckle_rows(self._h, min_faces, src.ptr, src.memkind, src.classes, ptr, mem))
        src.finish()
        return out

    def despeckle_sums(self, source, min_faces):
        """float32 [F,C]: the rows of `source` (an aggregator over the F faces, or float32 [F,C] rows) with every class of a removed
        face at 0; the rows of kept and of unlabelled faces pass through bit for bit."""
        return self._despeckle_sums(source, min_faces, False)

    def despeckle_sums_device(self, source, min_faces):
        """`despeckle_sums()` left in HBM: a `source` for `FaceGraph.fill_*`."""
        return self._despeckle_sums(source, min_faces, True)

    # ---- pooled rows, areas and the despeckle by a measure (include/smesh_segment_stats.h) ------------------------------------------
    # The pooled row of a segment is the float32 sum of its faces' rows (each times its face weight, where given) in ascending face
    # order: 256 faces to a chunk sum, the chunk sums one after another.  Two calls agree in every bit.  `source` is what it is for
    # `despeckle_sums`; `face_weights` and `measure` are float32 vectors, numpy or device.
    def _members(self, on_device):
        offsets, po, mem = _out((self.count + 1,), np.uint32, self.device, on_device)
        members, pm, mem = _out((self.num_labelled,), np.uint32, self.device, on_device)
        _lib.check(_lib.lib().smesh_segment_stats_members(self._h, po, pm, mem))
        return offsets, members

    def members(self):
        """`(offsets uint32[count+1], members uint32[num_labelled])`: the faces of segment s, ascending, are
        `members[offsets[s]:offsets[s+1]]`."""
        return self._members(False)

    def members_device(self):
        """`members()` left in HBM."""
        return self._members(True)

    def _areas(self, face_areas, on_device):
        streams = []
        pa, amem, keep = _dense_vector(face_areas, self.num_faces, "face_areas", "one element per face", self.device, streams)
        if pa is None:
            raise ValueError("face_areas is required")
        out, pout, omem = _out((self.count,), np.float32, self.device, on_device)
        _lib.check(_lib.lib().smesh_segment_stats_pool(self._h, pa, amem, 1, None, _lib.MEM_HOST, _lib.VTX_SUMS, 0.0, pout, None, omem))
        release_to(self.device, streams)
        return out

    def areas(self, face_areas):
        """float32 [count]: the area of every segment, `pool_sums(face_areas[:, None])[:, 0]`; `face_areas`: `FaceGraph.face_areas*()`."""
        return self._areas(face_areas, False)

    def areas_device(self, face_areas):
        """`areas()` left in HBM: a `measure` for `despeckle_*_by`."""
        return self._areas(face_areas, True)

    def _pool(self, source, face_weights, mode, threshold, want_labels, on_device, faces):
        streams = []
        pw, wmem, wkeep = _dense_vector(face_weights, self.num_faces, "face_weights", "one element per face", self.device, streams)
        src = _Source(source, self.num_faces, self.device, "the segments", "FaceSegments", streams)
        rows, labels, outs = _rows_and_labels(self.num_faces if faces else self.count, src.classes, self.device, not want_labels, want_labels,
                                              on_device)
        name = "pool_faces" if faces else "pool"
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(getattr(_lib.lib(), "smesh_aggregator_segment_stats_" + name)(source._h, self._h, pw, wmem, mode, float(threshold), *outs))
        else:
            _lib.check(getattr(_lib.lib(), "smesh_segment_stats_" + name)(self._h, src.ptr, src.memkind, src.classes, pw, wmem, mode,
                                                                          float(threshold), *outs))
        src.finish()
        return labels if want_labels else rows

    def pool_sums(self, source, face_weights=None):
        """float32 [count,C]: the pooled rows as they are."""
        return self._pool(source, face_weights, _lib.VTX_SUMS, 0.0, False, False, False)

    def pool(self, source, face_weights=None, dont_care_threshold=0.9):
        """float32 [count,C]: the pooled rows divided by their total; all-zero rows where the total is below `dont_care_threshold`."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, False, False)

    def pool_labels(self, source, face_weights=None, dont_care_threshold=0.9):
        """int32 [count]: the class with the largest pooled value (the lowest one among equals), -1 where don't care."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, False)

    def pool_sums_device(self, source, face_weights=None):
        """`pool_sums()` left in HBM."""
        return self._pool(source, face_weights, _lib.VTX_SUMS, 0.0, False, True, False)

    def pool_device(self, source, face_weights=None, dont_care_threshold=0.9):
        """`pool()` left in HBM."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, False)

    def pool_labels_device(self, source, face_weights=None, dont_care_threshold=0.9):
        """`pool_labels()` left in HBM."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, True, False)

    def pooled_face_sums(self, source, face_weights=None):
        """float32 [F,C]: every labelled face carries its segment's pooled row; an unlabelled face keeps its own row, unweighted."""
        return self._pool(source, face_weights, _lib.VTX_SUMS, 0.0, False, False, True)

    def pooled_face_annotations(self, source, face_weights=None, dont_care_threshold=0.9):
        """float32 [F,C]: `pooled_face_sums()` renormalised; all-zero rows where the total is below `dont_care_threshold`."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, False, True)

    def pooled_face_labels(self, source, face_weights=None, dont_care_threshold=0.9):
        """int32 [F]: region voting -- every face of a segment takes the label of the segment's pooled row, -1 where don't care."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, False, True)

    def pooled_face_sums_device(self, source, face_weights=None):
        """`pooled_face_sums()` left in HBM."""
        return self._pool(source, face_weights, _lib.VTX_SUMS, 0.0, False, True, True)

    def pooled_face_annotations_device(self, source, face_weights=None, dont_care_threshold=0.9):
        """`pooled_face_annotations()` left in HBM."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, False, True, True)

    def pooled_face_labels_device(self, source, face_weights=None, dont_care_threshold=0.9):
        """`pooled_face_labels()` left in HBM: a label table for `LabelRenderer`, `ConfusionMatrix.add*` and `PointTransfer`."""
        return self._pool(source, face_weights, _lib.VTX_ANNOTATIONS, dont_care_threshold, True, True, True)

    def _measure(self, measure, minimum, streams):
        if isinstance(minimum, bool) or not isinstance(minimum, (int, float, np.integer, np.floating)):
            raise ValueError("minimum must be a number, got %r" % (minimum,))
        pm, mmem, keep = _dense_vector(measure, self.count, "measure", "one element per segment", self.device, streams)
        if pm is None:
            raise ValueError("measure is required")
        return pm, mmem, keep, float(minimum)

    def _despeckle_labels_by(self, measure, minimum, return_removed, on_device):
        streams = []
        pm, mmem, keep, minimum = self._measure(measure, minimum, streams)
        out, ptr, mem = _out((self.num_faces,), np.int32, self.device, on_device)
        faces, segs = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(_lib.lib().smesh_segment_stats_despeckle_labels(self._h, pm, mmem, minimum, ptr, mem,
                                                                  ctypes.byref(faces) if return_removed else None,
                                                                  ctypes.byref(segs) if return_removed else None))
        release_to(self.device, streams)
        return (out, int(faces.value), int(segs.value)) if return_removed else out

    def despeckle_labels_by(self, measure, minimum, return_removed=False):
        """int32 [F]: `despeckle_labels()` with "kept" meaning `measure[segment] >= minimum` -- `measure`: float32 [count], e.g.
        `areas()` in square metres.  A NaN measure removes its segment.  `return_removed=True`: `(labels, removed faces, removed segments)`."""
        return self._despeckle_labels_by(measure, minimum, return_removed, False)

    def despeckle_labels_by_device(self, measure, minimum, return_removed=False):
        """`despeckle_labels_by()` left in HBM."""
        return self._despeckle_labels_by(measure, minimum, return_removed, True)

    def _despeckle_sums_by(self, source, measure, minimum, on_device):
        streams = []
        pm, mmem, keep, minimum = self._measure(measure, minimum, streams)
        src = _Source(source, self.num_faces, self.device, "the segments", "FaceSegments", streams)
        out, ptr, mem = _out((self.num_faces, src.classes), np.float32, self.device, on_device)
        if src.is_aggregator:
            # (`_h`: the aggregator's deferred views are handed to the library first, as get() does)
            _lib.check(_lib.lib().smesh_aggregator_segment_stats_despeckle(source._h, self._h, pm, mmem, minimum, ptr, mem))
        else:
            _lib.check(_lib.lib().smesh_segment_stats_despeckle_rows(self._h, pm, mmem, minimum, src.ptr, src.memkind, src.classes, ptr, mem))
        src.finish()
        return out

    def despeckle_sums_by(self, source, measure, minimum):
        """float32 [F,C]: `despeckle_sums()` with "kept" meaning `measure[segment] >= minimum`."""
        return self._despeckle_sums_by(source, measure, minimum, False)

    def despeckle_sums_by_device(self, source, measure, minimum):
        """`despeckle_sums_by()` left in HBM: a `source` for `FaceGraph.fill_*`."""
        return self._despeckle_sums_by(source, measure, minimum, True)
