"""The shared cases of tests/test_gpu_fuse_rows_instances.py and tests/test_fuse_rows_host.py: which instance of k_fuse_tri_labels,
k_fuse_tri_h16 and k_fuse_tri_sampled (fusion_labels.hip, fusion_half.hip, fusion_sampled.hip, over fuse_rows.inc.hpp) a launch must
be, the scenes that take each part of those kernels, the images, and the preconditions of every case computed from the CPU oracle.
numpy only, nothing read back from the library: the dispatch is restated here ONCE, from DESIGN.md 3.2 / 3.9, include/smesh_labels.h,
smesh_half.h and smesh_sampled.h and the comments of fuse_views_impl, narrow_plane and for_each_queued_triangle.

The rules:
  views          a fuse_views call goes through raster groups of eight; in each, fusion launches of the largest of 8 / 4 / 2 / 1 views
                 that fit what is left (`launches`).  The direct rasteriser (SMESH_RASTER=direct) renders view by view and hands its
                 views over two by two;
  slots          k_fuse_tri_h16 / k_fuse_tri_sampled: 1 .. 48 classes, register slots (C + 7) // 8 * 8; Sum / Summax: 6 x 2 x 4 = 48
                 instances each;
  label form     k_fuse_tri_labels<LT, NV, IN_LDS>: rows in LDS up to 255 classes, in global memory beyond; LT is uint16 from 256
                 classes on for every image the library narrows itself -- but a dense uint8 / uint16 image in DEVICE memory is its
                 own plane (narrow_plane: plane_in_place), whatever the class count.  So a uint16 image below 256 classes runs
                 <uint16_t, NV, true> and a uint8 image from 256 classes on <uint8_t, NV, false>: all 2 x 2 x 4 = 16 compiled
                 instances can be selected, not only the eight that the class count alone would pick, and LABEL_TABLE reaches all
                 of them (reported by the read-only option "last_fuse_labels_form": bytes per label, plus 16 for rows in LDS);
  tail walk      for_each_queued_triangle takes chunk = max(1, min(64, total // workers)) queue entries per step, workers = 16 x CUs,
                 total = the queue lengths of the launch's views, each capped by the queue capacity (the face count).

Scenes are helpers.small_scene grids seen from its ring of eight cameras; what each must offer is computed by `facts` and asserted by
test_fuse_rows_host.py.  Every builder is cached and returns read-only arrays.
"""
import collections
import functools
import inspect
import types

import numpy as np

import half_helpers as hh
import resize_ref as ref
import sampled_inputs as si
from helpers import small_scene

LABELS, H16, SAMPLED = KERNELS = ("k_fuse_tri_labels", "k_fuse_tri_h16", "k_fuse_tri_sampled")
W, H = 160, 120                      # every scene but "mid" and "capped"
CUS = 256                            # compute units of an MI355X (tests/image_kernels_scale_cases.py)
WORKERS = 16 * CUS                   # tail blocks of a launch (fuse_rows_grid)
WAVE = 64
SLOTS = (8, 16, 24, 32, 40, 48)
KINDS = ("sum", "summax")
VIEWS = (1, 2, 4, 8)
IEWS = (0.0, 0.5, 1.0)               # image_equal_weight
DTYPES = {H16: hh.DTYPES, SAMPLED: si.DTYPES, LABELS: ("uint8", "uint16")}
LDS_MAX_CLASSES = 255                # kLabelsLdsMaxC
SIZES = tuple(sorted(si.SOURCES))    # source sizes of the sampled kernel, by their names in sampled_inputs.SOURCES
REMAINDER_CLASSES = tuple(range(1, 9)) + tuple(range(41, 49))      # C mod 8 = 1 .. 7 and 0, in the first and in the last slot

# (name) -> small_scene(a, b, width, height), eight views each
SCENES = {"fine": (161, 79, W, H), "odd": (37, 19, W, H), "mid": (161, 79, 960, 720), "capped": (260, 130, 2240, 1680)}
# ... with a copy of the grid UNDER_DZ below it, faces appended: nearly all of the copy's fragments lose the depth test, so a triangle's
# coverage mask is its visible pixels only once the losers' bits are cleared -- or checked against the index plane (part D)
LAYERED = {"fine2": "fine", "odd2": "odd"}
UNDER_DZ = 0.4
# "mixed": the grid of "odd" seen by its ring of cameras, every second one from FAR_RADIUS times the ring's radius: the far views queue
# no triangle, the near ones queue many that the far ones show small (part E)
FAR_RADIUS = 3.0

# The views of a launch of 1 / 2 / 4 / 8: views 3 and 7 show a face in the image's last column and last rows, in "odd" views 3 and 7
# queue many triangles that the other shows small, and view 1 queues the most.
LAUNCH_VIEWS = {1: (3,), 2: (3, 7), 4: (0, 1, 2, 3), 8: tuple(range(8))}
TAIL_VIEWS = {**LAUNCH_VIEWS, 1: (1,)}
MIXED_VIEWS = {**LAUNCH_VIEWS, 2: (2, 3)}      # "mixed": a near and a far view in every launch from two views on

Case = collections.namedtuple("Case", "kernel slot kind views C dtype iew")


def case_id(c):
    return "%s-s%02d-%s-v%d-c%03d-%s-iew%g" % (c.kernel[len("k_fuse_tri_"):], c.slot, c.kind, c.views, c.C, c.dtype, c.iew)


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def slot(C):
    """Register slots of the k_fuse_tri_h16 / k_fuse_tri_sampled instance that takes C classes; 0 beyond the kernels."""
    return (C + 7) // 8 * 8 if 1 <= C <= 48 else 0


def launches(n, group_cap=8):
    """The views of every fusion launch of one fuse_views call of n views, in order."""
    out = []
    for start in range(0, n, 8):
        left = min(8, n - start)
        while left:
            nv = 1
            while nv * 2 <= min(group_cap, left):
                nv *= 2
            out.append(nv)
            left -= nv
    return out


def labels_form(dtype, C):
    """"last_fuse_labels_form" of a dense DEVICE label image of `dtype` (uint8 / uint16) at C classes."""
    return np.dtype(dtype).itemsize + (16 if C <= LDS_MAX_CLASSES else 0)


def instance(case, group_cap=8):
    """What the LAST launch of the case's call must report: (kernel, slot or label form, kind -- None for labels, which have one
    instance for both --, views)."""
    nv = launches(case.views, group_cap)[-1]
    if case.kernel == LABELS:
        return (LABELS, labels_form(case.dtype, case.C), None, nv)
    return (case.kernel, slot(case.C), case.kind, nv)


ALL_INSTANCES = frozenset({(k, s, kind, nv) for k in (H16, SAMPLED) for s in SLOTS for kind in KINDS for nv in VIEWS} |
                          {(LABELS, b + lds, None, nv) for b in (1, 2) for lds in (0, 16) for nv in VIEWS})


def chunk(total, workers=WORKERS):
    return max(1, min(WAVE, total // max(workers, 1)))


def steps(total, workers=WORKERS):
    """Steps of the tail walk; a worker takes a second one once there are more steps than workers."""
    return -(-total // chunk(total, workers))


# ---- part A / B: one case per instance ---------------------------------------------------------------------------------------------
def _class_vector_table(kernel):
    dts = DTYPES[kernel]
    out = []
    for i, s in enumerate(SLOTS):
        for k, kind in enumerate(KINDS):
            for v, nv in enumerate(VIEWS):
                C = (s - 7, s, s - 3)[(i + v) % 3]                   # the slot's low edge, its high edge, an odd remainder (5)
                out.append(Case(kernel, s, kind, nv, C, dts[(i + k + v) % len(dts)], IEWS[(i + k + 2 * v) % 3]))
    return out


def _label_table():
    out = []
    for i, (dtype, lds) in enumerate((("uint8", True), ("uint16", True), ("uint8", False), ("uint16", False))):
        for v, nv in enumerate(VIEWS):
            C = (5, 19, 150, 255)[(i + v) % 4] if lds else (256, 300)[(i + v) % 2]
            out.append(Case(LABELS, 0, KINDS[(i + v) % 2], nv, C, dtype, IEWS[(i + v) % 3]))
    return out


TABLE = tuple(_label_table() + _class_vector_table(H16) + _class_vector_table(SAMPLED))      # 16 + 48 + 48 cases


def size_of(case):
    """The source size (a key of sampled_inputs.SOURCES) of a sampled case: all three, dealt round."""
    return SIZES[(case.C + case.views + KINDS.index(case.kind)) % len(SIZES)]


# ---- part C: every remainder ---------------------------------------------------------------------------------------------------------
REMAINDER_TABLE = tuple(Case(k, slot(C), KINDS[(C + d) % 2], 2, C, dtype, IEWS[(C + d) % 3])
                        for k in (H16, SAMPLED) for d, dtype in enumerate(DTYPES[k]) for C in REMAINDER_CLASSES)


def four_corner_fraction(size):
    """The share of the (W,H) view pixels whose four bilinear taps are four DISTINCT source pixels (resize_ref.axis_table)."""
    w, h = si.SOURCES[size]
    x0, x1, _ = ref.axis_table(w, W)
    y0, y1, _ = ref.axis_table(h, H)
    return float((x0 != x1).mean() * (y0 != y1).mean())


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    """mesh, eight cameras and the ORACLE's index images of them."""
    from oracle import oracle
    a, b, w, h = SCENES[LAYERED.get(name, "odd" if name == "mixed" else name)]
    mesh, cams = small_scene(a, b, w, h, views=8)
    if name in LAYERED:
        under = mesh.vertices - np.array([0.0, 0.0, UNDER_DZ], np.float32)
        mesh = types.SimpleNamespace(vertices=np.concatenate([mesh.vertices, under]).astype(np.float32),
                                     faces=np.concatenate([mesh.faces, mesh.faces + len(mesh.vertices)]).astype(np.int32))
    if name == "mixed":
        from semantic_meshes_amd import synth
        near = inspect.signature(synth.ring_camera).parameters["radius_scale"].default          # (what small_scene's cameras have)
        cams = [cam if k % 2 == 0 else synth.ring_camera(k, 8, w, h, radius_scale=near * FAR_RADIUS) for k, cam in enumerate(cams)]
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    threads = oracle.get_threads()
    oracle.set_threads(8)
    try:
        oidx = tuple(_ro(o.render(cam)[0]) for cam in cams)
    finally:
        oracle.set_threads(threads)
    return types.SimpleNamespace(name=name, vertices=_ro(mesh.vertices), faces=_ro(mesh.faces), cams=tuple(cams), oidx=oidx, W=w, H=h)


def _extents(oi, P):
    """(lo, hi) int64 (P,2): the box of every face's VISIBLE pixels in one index image; hi = -1 where none is."""
    x, y = np.nonzero(oi < P)
    f = oi[x, y].astype(np.int64)
    lo = np.full((P, 2), 1 << 30, np.int64)
    hi = np.full((P, 2), -1, np.int64)
    for axis, coord in enumerate((x, y)):
        np.minimum.at(lo[:, axis], f, coord)
        np.maximum.at(hi[:, axis], f, coord)
    return lo, hi


@functools.lru_cache(maxsize=None)
def facts(name):
    """Per view and face, from the oracle's images and the float64 pinhole projection alone (test_gpu_half._boxes' rules):
      visible   some pixel shows the face;
      big       SURELY queued: its visible pixels alone span more than 8 in x or y (the rasteriser's box holds them);
      small     SURELY not queued: visible, and the projected vertices span at most 5 pixels either way;
      corner    visible at a pixel of the last column in one of the last eight rows (x = W-1, y >= H-8);
      span      the largest extent of visible pixels of any face, per view;
      hidden    layered scenes: faces of the copy underneath that show no pixel while the face above them shows some, per view."""
    sc = scene(name)
    P = len(sc.faces)
    v = np.asarray(sc.vertices, np.float64)
    tri = np.asarray(sc.faces)
    out = types.SimpleNamespace(visible=[], big=[], small=[], corner=[], span=[], hidden=[])
    for cam, oi in zip(sc.cams, sc.oidx):
        lo, hi = _extents(oi, P)
        vis = hi[:, 0] >= 0
        ext = np.where(vis[:, None], hi - lo + 1, 0)
        pc = v @ cam.rotation.astype(np.float64).T + cam.translation.astype(np.float64)
        assert (pc[:, 2] > 0).all()
        uv = pc[:, :2] / pc[:, 2:3] * cam.focal_lengths + cam.principal_point
        proj = (uv[tri].max(axis=1) - uv[tri].min(axis=1)).max(axis=1)
        corner = np.zeros(P, bool)
        last = oi[sc.W - 1, sc.H - 8:]
        corner[last[last < P]] = True
        half = P // 2          # (layered scenes: face f + half is face f's copy underneath)
        out.hidden.append(int((vis[:half] & ~vis[half:]).sum()) if name in LAYERED else 0)
        out.visible.append(vis)
        out.big.append(vis & (ext > 8).any(axis=1))
        out.small.append(vis & (proj <= 5.0))
        out.corner.append(corner)
        out.span.append(int(ext.max()))
    for key in ("visible", "big", "small", "corner"):
        setattr(out, key, _ro(np.array(getattr(out, key))))
    out.span, out.hidden = tuple(out.span), tuple(out.hidden)
    return out


def mixed_faces(name, views):
    """Faces that some view of `views` surely queues while another shows them without queueing them: the tail wave then scans the
    index plane of a view in which the triangle is small."""
    f = facts(name)
    views = list(views)
    big, small = f.big[views], f.small[views]
    return np.nonzero(big.any(axis=0) & small.any(axis=0))[0]


def entries_bounds(name, views=range(8)):
    """(least, most) queue entries of a launch of `views`: the surely queued faces, and every face in every view (the queue capacity)."""
    f = facts(name)
    return int(f.big[list(views)].sum()), len(list(views)) * len(scene(name).faces)


def decoy_views(views, n=8):
    """The views whose planes, records and queues sit in the view slots before a checked call: every camera one further round the ring."""
    return [(k + 1) % n for k in views]


def differing_fraction(name, k):
    sc = scene(name)
    return float((sc.oidx[k] != sc.oidx[(k + 1) % 8]).mean())


# ---- images ------------------------------------------------------------------------------------------------------------------------
def one_hot(labels, C):
    """tf.one_hot: float32 (W,H,C), the all-zero vector for a label outside [0, C)."""
    labels = np.asarray(labels).astype(np.int64)
    out = np.zeros(labels.shape + (C,), np.float32)
    ok = labels < C
    idx = np.nonzero(ok)
    out[idx + (labels[ok],)] = 1.0
    return out


@functools.lru_cache(maxsize=None)
def label_images(w, h, C, dtype, n=8):
    """n dense (w,h) label images of uint8 / uint16: classes 0 .. C-1 (those the dtype can hold), about 3 % of the pixels out of
    253 .. 257, C, C + 1 and the dtype's largest value -- at or above C: don't care, below: a class like any other."""
    rng = np.random.default_rng(31 * C + 7 * w + h + np.dtype(dtype).itemsize)
    top = np.iinfo(dtype).max
    out = []
    for _ in range(n):
        lab = rng.integers(0, min(C, top + 1), size=(w, h)).astype(np.int64)
        odd = rng.random((w, h)) < 0.03
        lab[odd] = rng.choice([253, 254, 255, 256, 257, C, C + 1, top], size=int(odd.sum()))
        out.append(_ro(np.minimum(lab, top).astype(dtype)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def h16_images(w, h, C, dtype, n=8):
    """(uint16 bit patterns, widened float32) of n images (half_helpers.random_probs16: don't-care rows, rows on either side of 0.5)."""
    rng = np.random.default_rng(1000 * C + 7 * hh.DTYPES.index(dtype) + w)
    img = [_ro(hh.random_probs16(rng, w, h, C, dtype)) for _ in range(n)]
    return tuple(img), tuple(_ro(hh.widen(i, dtype)) for i in img)


@functools.lru_cache(maxsize=None)
def sampled_images(w, h, C, dtype, size, n=8):
    """([(values, widened)] * n of the source size, [what the fusion must see at (w,h)] * n): sampled_inputs.source_images at the
    suites' 160 x 120, the same construction at another view size (the source then 0.37 of the view)."""
    if (w, h) == (W, H):
        small, big = si.source_images(C, dtype, si.SOURCES[size], n)
    else:
        sw, sh = int(0.37 * w), int(0.37 * h)
        rng = np.random.default_rng(77 * C + 13 * sw + si.DTYPES.index(dtype))
        small, big = [], []
        for _ in range(n):
            if dtype == "float32":
                from helpers import random_probs
                values = wide = random_probs(rng, sw, sh, C)
            else:
                b = hh.random_probs16(rng, sw, sh, C, dtype)
                values, wide = hh.typed(b, dtype), hh.widen(b, dtype)
            small.append((values, wide))
            big.append(si.seen(ref.ref_resize(wide, w, h), dtype))
    return tuple((_ro(v), _ro(x)) for v, x in small), tuple(_ro(b) for b in big)


@functools.lru_cache(maxsize=None)
def weight_images(w, h, n=8):
    """n float32 (w,h) weights images, a tenth of the pixels zero."""
    rng = np.random.default_rng(99 + w)
    out = []
    for _ in range(n):
        x = rng.uniform(0.1, 2.0, size=(w, h)).astype(np.float32)
        x[rng.random((w, h)) < 0.1] = 0.0
        out.append(_ro(x))
    return tuple(out)


def release_images():
    """Forget every cached image (the large scenes' are hundreds of megabytes); the small ones are rebuilt when next asked for."""
    for builder in (label_images, h16_images, sampled_images, weight_images):
        builder.cache_clear()


# ---- part G: label images of odd sizes ------------------------------------------------------------------------------------------------
EDGE_SIZES = {(7, 3): (8, 4), (9, 1000): (161, 79), (1000, 9): (161, 79), (33, 65): (40, 20)}       # image size -> grid of the mesh


@functools.lru_cache(maxsize=None)
def edge_scene(size):
    """A grid seen by two ring cameras whose focal lengths are those of the 160 x 120 scenes PER AXIS (0.8 W, 0.8 x 4/3 H), so that
    the mesh fills an image of any aspect as it fills those."""
    from oracle import oracle
    from semantic_meshes_amd.data import Camera
    w, h = size
    a, b = EDGE_SIZES[size]
    mesh, ring = small_scene(a, b, w, h, views=2)
    cams = tuple(Camera(c.rotation, c.translation, np.asarray([w, h]), np.asarray([0.8 * w, 0.8 * 4.0 / 3.0 * h]),
                        np.asarray([w / 2.0, h / 2.0])) for c in ring)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    oidx = tuple(_ro(o.render(cam)[0]) for cam in cams)
    return types.SimpleNamespace(name="edge %dx%d" % size, vertices=_ro(mesh.vertices), faces=_ro(mesh.faces), cams=cams, oidx=oidx, W=w, H=h)
