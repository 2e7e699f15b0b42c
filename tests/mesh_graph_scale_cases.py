"""The shared cases of tests/test_gpu_mesh_graph_scale.py and tests/test_mesh_graph_scale_host.py: meshes past the sizes at which the
mesh-graph kernels change their launches, label patterns on them, and the references of both.  A plain helper module, no conftest:
every builder is cached, every array it returns is read-only, so a reference is computed once per session whoever asks first.

Every reference comes from tests/face_graph_ref.py, tests/face_segments_ref.py and tests/points_ref.py, never from the library.

The two sizes the cases are built around (restated here, not read from the library):
  SCAN_CHUNK   256 * 1024   k_scan_sums (scan.inc.hpp) scans the tile totals kBlock = 256 at a time, a tile is kScanTile = 1024
                            elements: a scan of more elements has a second chunk and needs the carry;
  CAPPED_GRID  2048 * 256   kCountBlocks * kBlock (face_segments.hip): the lanes of the capped grid of k_seg_flatten,
                            k_seg_despeckle_labels and k_seg_small; more items than that and a lane takes a second one."""
import functools

import numpy as np

import face_graph_ref as gref
import face_segments_ref as sref
import points_ref
import test_gpu_face_graph as tgf
import test_gpu_face_segments as tfs

SCAN_CHUNK = 256 * 1024          # kBlock * kScanTile of scan.inc.hpp
CAPPED_GRID = 2048 * 256         # kCountBlocks * kBlock of face_segments.hip

GRID = (530, 500)                # synth.grid_mesh(530, 500): F = 530 000, V = 266 031
BIG_F, BIG_V = 530000, 266031
# F + 1 is what the graph and the segments scan, and what k_seg_flatten strides over: the last size without a second scan chunk and
# the first with one, the last size inside the capped grid and the first beyond it
EDGE_FACES = (SCAN_CHUNK - 1, SCAN_CHUNK, CAPPED_GRID - 1, CAPPED_GRID)
# V + 1 is what the vertex map scans: the same edge, and the big grid's own V
VERTEX_COUNTS = (SCAN_CHUNK - 1, SCAN_CHUNK, BIG_V)
SHUFFLE_SEED = 530500            # the one permutation of the shuffled grid
THRESHOLD = 0.9
POINTS = 16

GRAPH_CASES = ("big", "shuffled") + tuple("first%d" % F for F in EDGE_FACES)
BIG_PATTERNS = ("constant", "serpentine", "blocks32_noisy", "random2")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def big_mesh():
    """(faces int32[F,3], vertices float32[V,3]) of the big grid."""
    from semantic_meshes_amd import synth
    mesh = synth.grid_mesh(*GRID)
    faces, vertices = np.ascontiguousarray(mesh.faces, np.int32), mesh.vertices.astype(np.float32).copy()
    assert faces.shape == (BIG_F, 3) and vertices.shape == (BIG_V, 3)
    return _frozen(faces, vertices)


@functools.lru_cache(maxsize=None)
def permutation():
    """(perm, inverse): face i of the shuffled grid is face perm[i] of the big grid."""
    perm = np.random.default_rng(SHUFFLE_SEED).permutation(BIG_F)
    inverse = np.empty(BIG_F, np.int64)
    inverse[perm] = np.arange(BIG_F)
    return _frozen(perm, inverse)


@functools.lru_cache(maxsize=None)
def case(name):
    """(faces, vertices, V, offsets, neighbours) as test_gpu_face_graph._case gives them, the adjacency by face_graph_ref.
    "big"; "shuffled": the big grid's faces in the seeded permutation, a face order that is not spatially coherent; "first<F>": the
    first F faces of the big grid over all of its vertices; "isolated": 530 000 triangles that share nothing."""
    if name == "isolated":
        faces = np.arange(3 * BIG_F, dtype=np.int32).reshape(BIG_F, 3)
        out = tgf._case(faces, np.zeros((3 * BIG_F, 3), np.float32))
        assert len(out[4]) == 0
        return out
    faces, vertices = big_mesh()
    if name == "shuffled":
        faces = np.ascontiguousarray(faces[permutation()[0]])
    elif name.startswith("first"):
        faces = np.ascontiguousarray(faces[:int(name[5:])])
    elif name != "big":
        raise KeyError(name)
    return tgf._case(faces, vertices)


@functools.lru_cache(maxsize=None)
def vertex_case(V):
    """(faces, V): the faces of the big grid that name no vertex >= V."""
    faces, _ = big_mesh()
    n = BIG_F if V >= BIG_V else int(np.argmax(faces.max(axis=1) >= V))      # (the largest index never falls along the face order)
    sub = np.ascontiguousarray(faces[:n])
    assert n > 0 and sub.max() < V and (n == BIG_F or faces[n:].max(axis=1).min() >= V)
    return _frozen(sub)[0], V


# ---- label patterns ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def labels(name, pattern):
    """int32 [F].  On "big" the patterns of test_gpu_face_segments at GRID; on "shuffled" the same labels on the same triangles, so the
    segments are the same sets of triangles, numbered otherwise; on "first<F>" random2; on "isolated" constant, or every seventh -1."""
    a, b = GRID
    if name == "shuffled":
        out = labels("big", pattern)[permutation()[0]]
    elif name == "isolated":
        out = np.full(BIG_F, 5, np.int32)
        if pattern == "seventh":
            out[::7] = -1
        elif pattern != "constant":
            raise KeyError(pattern)
    elif name.startswith("first"):
        assert pattern == "random2"
        out = tfs.random_labels(int(name[5:]) % 1000, int(name[5:]), 2)
    elif pattern == "constant":
        out = np.full(BIG_F, 5, np.int32)
    elif pattern == "serpentine":
        out = tfs.serpentine(a, b)
    elif pattern == "blocks32_noisy":                                        # tools/face_segments_bench.py's blocks_3pct_noise
        rng = np.random.default_rng(0)
        out = tfs.blocks(a, b, 32, 19)
        hit = rng.random(BIG_F) < 0.03
        out[hit] = rng.integers(0, 19, int(hit.sum()))
    elif pattern == "random2":                                               # 10 % of the faces at -1
        out = tfs.random_labels(2, BIG_F, 2)
    else:
        raise KeyError(pattern)
    out = np.ascontiguousarray(out, np.int32)
    assert out.shape == (len(case(name)[0]),)
    return _frozen(out)[0]


@functools.lru_cache(maxsize=None)
def entry_weights(name, kind):
    """(weights float32[nnz], min_weight), by the recipes of test_gpu_face_segments.entry_weights."""
    faces, vertices, V, offsets, nbr = case(name)
    if kind == "normal":
        w, min_weight = gref.normal_weights(offsets, nbr, vertices, faces), 0.5
    elif kind == "asymmetric":                                               # every entry on its own: most edges pass one way only or not at all
        w, min_weight = np.random.default_rng(77).random(len(nbr), dtype=np.float32), 0.6
    else:
        raise KeyError(kind)
    return _frozen(w)[0], min_weight


@functools.lru_cache(maxsize=None)
def expected(name, pattern, kind=None):
    """The flood fill's (ids, first_face, label, size)."""
    faces, vertices, V, offsets, nbr = case(name)
    w, min_weight = entry_weights(name, kind) if kind else (None, None)
    return _frozen(*sref.segments(offsets, nbr, labels(name, pattern), w, min_weight))


# ---- propagation on the big grid ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(C, seed):
    """float32 [F,C] on the big grid: 30 % of the rows all zero, a tenth with a total of 0.3 (below the threshold), the others 1."""
    rng = np.random.default_rng(seed)
    x = (rng.random((BIG_F, C), dtype=np.float32) ** 3 + np.float32(1e-3)).astype(np.float32)
    x /= x.sum(axis=1, keepdims=True)
    kind = rng.random(BIG_F)
    x[kind < 0.3] = 0.0
    x[kind > 0.9] *= np.float32(0.3)
    return _frozen(x)[0]


@functools.lru_cache(maxsize=None)
def propagated(mode):
    """(rows, weights or None, x_2, tot_2): two iterations on the big grid -- FILL at 19 classes without weights, SMOOTH at 40 classes
    with the normal weights."""
    faces, vertices, V, offsets, nbr = case("big")
    if mode == gref.FILL:
        x0, w = rows(19, 19), None
    else:
        x0, w = rows(40, 40), entry_weights("big", "normal")[0]
    x, tot = gref.propagate(offsets, nbr, x0, 2, mode, alpha=0.5, observed_threshold=THRESHOLD, weights=w)
    return (x0, w) + _frozen(x, tot)


# ---- points near the big grid ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def near_points():
    """(points float32[POINTS,3], (faces, dist2) of the exhaustive reference): seeded points within 0.01 of the big grid's surface."""
    faces, vertices = big_mesh()
    rng = np.random.default_rng(16)
    pick = rng.integers(0, BIG_F, POINTS)
    bary = rng.dirichlet(np.ones(3), POINTS)[:, :, None]
    step = rng.normal(size=(POINTS, 3))
    step *= (0.01 * rng.random(POINTS) / np.linalg.norm(step, axis=1))[:, None]
    points = ((vertices[faces[pick]].astype(np.float64) * bary).sum(axis=1) + step).astype(np.float32)
    want = points_ref.nearest(vertices, faces, points, chunk=4)
    return _frozen(points)[0], _frozen(*want)
