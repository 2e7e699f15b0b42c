"""The shared cases of tests/test_gpu_image_kernels_scale.py and tests/test_image_kernels_scale_host.py: images past the sizes at
which the image-side kernels change their launches, and the references of them.  A plain helper module, no conftest: every builder
is cached, every array it returns is read-only, so an image and its reference are computed once per session whoever asks first.

Every reference comes from tests/probs_labels_ref.py, tests/depth_gate_ref.py, tests/edge_gate_ref.py, tests/label_prep_ref.py,
tests/label_colors_ref.py and tests/resize_ref.py, never from the library.  (The planes of the view-weights and fusion tests are
renders, which need the device: tests/test_gpu_image_kernels_scale.py makes them and takes their expectations from
tests/view_weights_ref.py, depth_gate_ref and edge_gate_ref; here are only their sizes.)

The thresholds the cases are built around (restated here, not read from the library):
  STAGE_WORDS   6144   kStageWords (probs_labels.hip): a tile of k_probs_labels_tiled holds min(PL_BLOCK, 6144 // (C | 1)) pixels;
  PL_BLOCK      256    kPlBlock (probs_labels.hip): lanes of a workgroup, and the pixels of one round of k_probs_labels_generic;
  GROUPS_PLAIN  6      kGroupsPerCuPlain / kGroupsPerCuCount (probs_labels.hip): launch_probs_labels caps the grid at this many
  GROUPS_COUNT  4      workgroups per CU; past the cap a workgroup takes a second tile (round), and a third ...;
  CHUNK         4096   kChunk (depth_weights.hip, view_weights.hip): output pixels of one workgroup;
  XCDS          8      kXcds (depth_weights.hip, view_weights.hip): the grid is a multiple of it, and with grid / 8 >= 2 the chunks
                       are dealt to the workgroups in runs (a permutation), below that in order;
  TILE_X, _Y    32, 64 SMESH_EDGE_TILE_X / _Y (include/smesh_edge_gate.h): a workgroup of k_edge_weights; a group launch has the
                       columns of its widest and the rows of its tallest view;
  NEAREST_64    2^32   src_index (nearest_rule.hpp; label_colors.hip has its own copy): (2X + 1) n at or above it is divided in
                       64 bits, below it in 32;
  MAX_GRID_Y    65535  kMaxGridY (resize.hip): the resize kernels have one blockIdx.y per output column up to this many; column
                       65535 of an image 65536 wide is the second turn of workgroup 0's loop.
CUS = 256 is the MI355X's: the probs-labels shapes are computed for it, and the GPU test asserts from the launch's own report
(the read-only options "last_probs_labels_grid" / "last_probs_labels_work") that they did what they are for."""
import functools

import numpy as np

import depth_gate_ref as dg
import edge_gate_ref as eg
import label_colors_ref as lc
import label_prep_ref as lp
import probs_labels_ref as pl
import resize_ref as rs

STAGE_WORDS = 6144               # kStageWords of probs_labels.hip
PL_BLOCK = 256                   # kPlBlock of probs_labels.hip
GROUPS_PLAIN, GROUPS_COUNT = 6, 4   # kGroupsPerCuPlain, kGroupsPerCuCount of probs_labels.hip
CHUNK = 4096                     # kChunk of depth_weights.hip and view_weights.hip
XCDS = 8                         # kXcds of depth_weights.hip and view_weights.hip
TILE_X, TILE_Y = 32, 64          # SMESH_EDGE_TILE_X, SMESH_EDGE_TILE_Y of include/smesh_edge_gate.h
NEAREST_64 = 1 << 32             # src_index of nearest_rule.hpp: (2X + 1) n from here on takes the 64-bit division
MAX_GRID_Y = 65535               # kMaxGridY of resize.hip
CUS = 256                        # compute units of an MI355X

THRESHOLDS = (None, 0.9)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A. the probs-labels loops ---------------------------------------------------------------------------------------------------
# name -> (classes, dtype, (W,H), layouts of test_gpu_probs_labels.device_layout, counting).  The shapes are the smallest round ones
# with 2.25 cap < work < 3 cap at 256 CUs: three rounds, the third for only some of the workgroups.
PL_CASES = {
    # 24 rows per tile; 83 100 pixels are 3 463 tiles (the last of 12 pixels) for 1 536 workgroups.  84.8 MB.
    "dense255": (255, "float32", (300, 277), ("dense", "permuted", "offset"), False),
    # runs of 98 pixels: five tiles of 24, 24, 24, 24 and 2 pixels each, 3 600 tiles.  The tiles b, b + 1 536, b + 3 072 of a workgroup
    # stand at different places of runs 307 or 308 apart, whose bases (3 elements of padding) differ in alignment.  72 MB / 36 MB.
    "rows255": (255, "float32", (720, 98), ("padded rows",), False),
    "rows255 permuted": (255, "float16", (98, 720), ("padded rows permuted",), False),
    # 97 rows per tile; 225 600 pixels are 2 326 tiles for 1 024 counting workgroups.  57 MB / 28 MB.
    "count63 float32": (63, "float32", (480, 470), ("dense",), True),
    "count63 float16": (63, "float16", (480, 470), ("dense",), True),
    # the workload's class counts: 256 and 149 rows per tile, 3 461 and 3 464 tiles
    "dense19": (19, "float16", (1000, 886), ("dense",), False),
    "dense40": (40, "float16", (800, 645), ("dense",), False),
    # the generic path: 3 461 rounds of 256 pixels, for 1 536 workgroups plain and 1 024 counting
    "generic3": (3, "float32", (1000, 886), ("channel first",), False),
    "generic3 bfloat16": (3, "bfloat16", (1000, 886), ("class stride 2",), False),
    "generic3 counting": (3, "float32", (1000, 886), ("channel first", "class stride 2"), True),
}
COUNT_GT_DTYPES = ("uint8", "uint16")     # MODE 1 and MODE 2 of k_probs_labels_tiled
TILEABLE = ("dense", "permuted", "offset", "padded rows", "padded rows permuted")


def pl_cap(counting, cus=CUS):
    """The largest grid of launch_probs_labels."""
    return cus * (GROUPS_COUNT if counting else GROUPS_PLAIN)


def pl_tile_pixels(C):
    """npix of plan_tiles: pixels of a full tile."""
    return min(PL_BLOCK, STAGE_WORDS // (C | 1))


def pl_work(name, layout):
    """("tiled" | "generic", work) of a case in a layout, by the rules of plan_tiles: tiles -- a contiguous image is ONE run, an image
    of padded rows has a run per row, each with a last tile of its own -- or rounds of 256 pixels."""
    C, dtype, (W, H), layouts, counting = PL_CASES[name]
    assert layout in layouts
    if layout not in TILEABLE:
        return "generic", -(-(W * H) // PL_BLOCK)
    npix = pl_tile_pixels(C)
    if layout == "padded rows":
        runs, L = W, H
    elif layout == "padded rows permuted":
        runs, L = H, W
    else:
        runs, L = 1, W * H
    assert runs == 1 or L * 8 >= npix       # (kMinRunShare: shorter runs would go to the generic path)
    return "tiled", runs * -(-L // npix)


@functools.lru_cache(maxsize=None)
def pl_image(C, dtype, shape):
    """(values, widened, {threshold: (labels, don't care)}) of one seeded image of probs_labels_ref.make_probs."""
    rng = np.random.default_rng([C, pl.DTYPES.index(dtype), shape[0], shape[1], 2])
    vals, wide, planted = pl.make_probs(rng, shape[0], shape[1], C, dtype)
    want = {}
    for t in THRESHOLDS:
        want[t] = _frozen(*pl.ref_labels(wide, t))
    _frozen(vals, wide)
    return vals, wide, want


def pl_case_image(name):
    C, dtype, shape, layouts, counting = PL_CASES[name]
    return pl_image(C, dtype, shape)


@functools.lru_cache(maxsize=None)
def pl_ground_truth(C, shape, gt_dtype):
    """Ground truth as probs_labels_ref.make_gt plants it: about 3 % out of range."""
    rng = np.random.default_rng([C, shape[0], shape[1], pl.LBL_DTYPES.index(gt_dtype)])
    return _frozen(pl.make_gt(rng, shape, C, gt_dtype))[0]


@functools.lru_cache(maxsize=None)
def pl_matrix(name, gt_dtype, threshold):
    """(M uint64 [C, C + 1], ignored): np.add.at over the reference labels of a counting case."""
    C, dtype, shape, layouts, counting = PL_CASES[name]
    lab, dc = pl_case_image(name)[2][threshold]
    M, ignored = pl.expected_matrix(np.where(dc, -1, lab), pl_ground_truth(C, shape, gt_dtype), C)
    return _frozen(M)[0], ignored


# ---- B. depth and view weights in runs per XCD -----------------------------------------------------------------------------------
PLANES = ((283, 251), (211, 173))         # 71 033 pixels (N mod 4 == 1): 18 chunks, grid 24, 3 per XCD; 36 503: 9 chunks, grid 16, 2 per XCD
SENSOR_SHAPES = {(283, 251): (283, 251), (211, 173): (160, 120)}      # the sensor at the plane's size, and at its own
GROUP_SIZES = ((283, 251), (96, 64))      # inside one group: the grid comes from the large view, 2 chunks of 24 serve the small one
GROUP_SENSOR = (160, 120)
GROUP_VIEWS = 9                           # a full group of eight and one more


def chunks(size):
    return -(-(size[0] * size[1]) // CHUNK)


def xcd_grid(size):
    """gridDim.x of k_depth_weights / k_view_weights for a launch whose largest view has `size`."""
    return XCDS * -(-chunks(size) // XCDS)


def per_xcd(size):
    return xcd_grid(size) // XCDS


def xcd_chunk(block, grid):
    """The chunk workgroup `block` of a grid takes: ((b mod 8) per_xcd + b div 8)."""
    return (block % XCDS) * (grid // XCDS) + block // XCDS


# ---- C. the edge gate with unlike tile grids in one launch -----------------------------------------------------------------------
EDGE_SIZES = ((40, 130), (100, 30))       # 2 x 3 and 4 x 1 tiles: the launch has 4 x 3, the widest and the tallest view differ
# (a pixel of these narrow views spans 0.1 to 0.2 m of the scene, so the tolerances are looser than the sibling tests': with theirs two
#  of the nine views keep no pixel at all; with these every view keeps some and loses some)
EDGE_GATES = ((3, 0.5, 0.02, True, True, True), (8, 2.0, 0.0, True, True, True))


def tile_grid(size):
    return -(-size[0] // TILE_X), -(-size[1] // TILE_Y)


def launch_tile_grid(sizes):
    """(columns of the widest, rows of the tallest) view: the grid of a group launch of k_edge_weights."""
    return max(tile_grid(s)[0] for s in sizes), max(tile_grid(s)[1] for s in sizes)


# ---- D. sides over 32 768 --------------------------------------------------------------------------------------------------------
LONG_SOURCE, LONG_TARGET = 40000, 65536   # (2X + 1) 40 000 >= 2^32 from X = 53 687 on
LONG_AXES = (0, 1)                        # (40000, 1) -> (65536, 1), and (1, 40000) -> (1, 65536)
LONG_CLASSES = (5, 300)                   # a uint8 and a uint16 plane
LONG_MAP = 1358


def long_shape(n, axis):
    return (n, 1) if axis == 0 else (1, n)


@functools.lru_cache(maxsize=None)
def long_labels(axis, C, with_map):
    """(source int32, map or None, the plane label_prep_ref.prepare gives): independent values pixel by pixel, so that a wrong source
    index shows."""
    rng = np.random.default_rng([40000, axis, C, int(with_map)])
    m = lp.make_map(rng, LONG_MAP, C) if with_map else None
    src = lp.make_source(rng, *long_shape(LONG_SOURCE, axis), np.int32, LONG_MAP if with_map else C)
    want = lp.prepare(src, C, long_shape(LONG_TARGET, axis), m)
    return _frozen(src)[0], (None if m is None else _frozen(m)[0]), _frozen(want)[0]


@functools.lru_cache(maxsize=None)
def long_colors(axis, C):
    """(colour image uint8 (w,h,3), colours (256,3), classes [256], the plane label_colors_ref.prepare gives)."""
    rng = np.random.default_rng([40000, axis, C, 3])
    colors = lc.make_palette(rng, 256)
    cls = lp.make_map(rng, 256, C).astype(np.int64)
    src = lc.make_image(rng, *long_shape(LONG_SOURCE, axis), colors, 3, absent=0.3)
    want = lc.prepare(src, C, long_shape(LONG_TARGET, axis), colors, cls)
    return _frozen(src, colors, cls, want)


LONG_GATE = (0.02, 0.0, None, None, "drop")


@functools.lru_cache(maxsize=None)
def long_depth(axis, dtype):
    """(depth plane float32, sensor image, weights-in, (weights, counts) of depth_gate_ref.weights): sensor samples independent from
    pixel to pixel between 1 and 6 metres (a tenth missing); seven in ten depths equal the sample the rule picks for them, the others
    are half a metre off or background -- so a wrong source index turns a kept pixel into an inconsistent one almost surely."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([40000, axis, 7 if dtype == np.float32 else 0])
    shape, target = long_shape(LONG_SOURCE, axis), long_shape(LONG_TARGET, axis)
    mm = rng.integers(1000, 6000, size=shape)
    sensor = mm.astype(np.uint16) if dtype == np.uint16 else (mm.astype(np.float32) * np.float32(0.001)).astype(np.float32)
    sensor[rng.random(shape) < 0.1] = 0
    g = dg.gate(*LONG_GATE, dtype=dtype)
    depth = (dg.sample(sensor, *target).astype(np.float32) * g.scale).astype(np.float32)
    kind = rng.random(target)
    depth[kind < 0.2] += np.float32(0.5)
    depth[kind > 0.95] = np.inf
    w_in = rng.uniform(0.1, 2.0, size=target).astype(np.float32)
    want, counts = dg.weights(depth, sensor, g, w_in)
    return _frozen(depth, sensor, w_in) + (_frozen(want, counts),)


# ---- E. width 65 536 through the resize kernels ----------------------------------------------------------------------------------
WIDE_SOURCE, WIDE_TARGET = (1000, 2), (65536, 2)
WIDE_LABEL_CLASSES = 19                   # with 16-byte pieces: four of four classes and a tail of three


@functools.lru_cache(maxsize=None)
def wide_source(C, dtype):
    """(values, widened) of resize_ref.make_source at WIDE_SOURCE."""
    rng = np.random.default_rng([1000, 2, C, rs.DTYPES.index(dtype)])
    return _frozen(*rs.make_source(rng, *WIDE_SOURCE, C, dtype))


@functools.lru_cache(maxsize=None)
def wide_resized(C, dtype):
    """resize_ref.ref_resize of that image: float32 (65536, 2, C)."""
    return _frozen(rs.ref_resize(wide_source(C, dtype)[1], *WIDE_TARGET))[0]


@functools.lru_cache(maxsize=None)
def wide_label_source(dtype):
    """(values, widened) of probs_labels_ref.make_probs at WIDE_SOURCE: rows with sums on both sides of 0.9."""
    rng = np.random.default_rng([1000, 2, WIDE_LABEL_CLASSES, rs.DTYPES.index(dtype), 1])
    vals, wide, _ = pl.make_probs(rng, *WIDE_SOURCE, WIDE_LABEL_CLASSES, dtype)
    return _frozen(vals, wide)


@functools.lru_cache(maxsize=None)
def wide_labels(dtype, threshold):
    """(labels, don't care) of the resampled image."""
    big = rs.ref_resize(wide_label_source(dtype)[1], *WIDE_TARGET)
    return _frozen(*pl.ref_labels(big, threshold))


# ---- the edge planes of the host test --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_plane(size):
    """A seeded plane of edge_gate_ref.random_plane at one of EDGE_SIZES (the GPU test gates renders; this one lets the host test
    hold the two forms of the restatement against each other at the same sizes)."""
    rng = np.random.default_rng([size[0], size[1]])
    depth = eg.random_plane(rng, *size)
    w_in = rng.uniform(0.1, 2.0, size=size).astype(np.float32)
    return _frozen(depth, w_in)
