"""The shared cases of tests/test_gpu_raster_instances.py and tests/test_raster_instances_host.py: which instance of the rasteriser
(semantic_meshes_amd/csrc/raster.hip) a launch must be, and the smallest scenes that make the library pick each one by itself.
Plain numpy, no library import: the dispatch is restated here ONCE, from DESIGN.md 3.1 / 5 and the comments of raster_args,
want_spread, frag_groups, render_into and render_group_into, and never read back from the library.  The GPU module asserts every
launch against it through the read-only options "last_raster_kernel" / "_mode" / "_views" / "_tpw" / "_groups" / "_chunk" / "_stages".

The rules (a camera is a `Cam`; `b` the mesh's summary, `bounds()`):
  typical edge   mean edge x max(|fx|, |fy|) / depth of the centre of the mesh's box; 0 where that depth is <= 1e-3;
  depth spread   farthest over nearest depth of the box's corners; +inf where the nearest is <= 1e-3 of the farthest; 1 behind the camera;
  MODE           bit 0 wg_push: typical edge >= 5;  bit 1 spread waves (always with bit 0): ONE view, spread <= 6, edge 10.5 .. 19;
                 bit 2 texel primitives;  bit 3 packed fragments: triangle primitives, F <= 2^22, option "packed_fragments";
  balance        depth spread > 6; the medium stage (k_raster_medium) is launched iff balance and (MODE & 3) != 0;
  votes          a grouped launch turns wg_push / balance (and spread, which no view of a group asks for) on iff
                 2 x votes >= n and votes > 0 -- a tie turns it on -- and the minority runs in the majority's instance;
  meshlets       a grouped launch with (MODE & 3) == 0, the renderer's tables (every block of 256 faces within 384 distinct vertices)
                 and the option "raster_meshlets": k_raster_frag_group_ml, 64 triangles per wave, no vertex stage;
  tpw            64, halved while launch_views x F / tpw < min_waves (integer division): F < 32 768: 2 048 waves, one view counted;
                 else 1 024 waves, every view of the launch counted; spread waves: 7.  So 1 below 4 096 faces, 2 / 4 / 8 up to
                 8 192 / 16 384 / 32 768, then 32 for ONE view below 65 536 and 64 otherwise: the ladder never stops at 16, so no case
                 can stand there (test_raster_instances_host.py sweeps the face counts);
  groups         1 unless tpw == 64 and F >= 4e6 (SMESH_RASTER_GROUPS forces: hook only);
  chunk          8 (kRasterXcdRun) once the launch has 64 blocks of four waves per view, else 0;
  huge stage     launched unless box_extent_bound proves every box within 60 pixels and in front of the near plane;
  compact        8-byte records: fuse_views of a triangle renderer in the caller's face order into a k_fuse_tri aggregator, the option
                 "compact_records", no depth planes; render() and everything else: 16.
"""
import collections
import functools
import math
import types

import numpy as np

XCD_RUN = 8                      # kRasterXcdRun
LANE_BOX, LANE_BOX_MIN = 24, 20  # kLaneBox, kLaneBoxMin: boxes of 9 .. 24 a lane walks itself where a wave holds 20 of them
MEDIUM = 64                      # kMedium: larger boxes (and near-plane crossings) go to the tile workgroups, k_raster_huge
SPREAD_TRIS = 7                  # kSpreadTris: triangles of a spread wave
PACKED_MAX_F = 1 << 22           # kFragMaxPrimitives
MESHLET_TRIS, MESHLET_MAX_VERTS = 256, 384
MARGIN = 0.2                     # every estimate lies this far (relative) from each threshold it is meant to be on one side of
C = 19

Cam = collections.namedtuple("Cam", "R t W H fx fy cx cy")
NO_KNOBS = types.MappingProxyType({"spread": -1, "wg_push": -1, "balance": -1, "groups": 0})
KERNELS = {0: "none", 1: "k_raster_frag", 2: "k_raster_frag_group", 3: "k_raster_frag_group_ml", 4: "direct"}
FIELDS = ("kernel", "mode", "views", "tpw", "groups", "chunk", "stages")


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def bounds(vertices, faces):
    """mesh_bounds: box of the float32 vertices, mean and longest edge of the faces, in double."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces)
    e = np.concatenate([np.linalg.norm(v[f[:, k]] - v[f[:, (k + 1) % 3]], axis=1) for k in range(3)])
    return types.SimpleNamespace(lo=v.min(0), hi=v.max(0), mean_edge=float(e.mean()), max_edge=float(e.max()))


def _corner_depths(b, cam):
    R, t = np.asarray(cam.R, np.float32).astype(np.float64), np.asarray(cam.t, np.float32).astype(np.float64)
    return [t[2] + sum(R[2, d] * (b.hi[d] if (c >> d) & 1 else b.lo[d]) for d in range(3)) for c in range(8)]


def typical_edge_pixels(b, cam):
    R, t = np.asarray(cam.R, np.float32).astype(np.float64), np.asarray(cam.t, np.float32).astype(np.float64)
    z = t[2] + float(R[2] @ (0.5 * (b.lo + b.hi)))
    if not z > 1e-3 or not b.mean_edge > 0:
        return 0.0
    return b.mean_edge * max(abs(cam.fx), abs(cam.fy)) / z


def depth_spread(b, cam):
    z = _corner_depths(b, cam)
    if not max(z) > 0:
        return 1.0
    return max(z) / min(z) if min(z) > 1e-3 * max(z) else math.inf


def box_extent_bound(b, cam):
    R, t = np.asarray(cam.R, np.float32).astype(np.float64), np.asarray(cam.t, np.float32).astype(np.float64)
    mag = max(abs(t[r]) + sum(abs(R[r, d]) * max(abs(b.lo[d]), abs(b.hi[d])) for d in range(3)) for r in range(3))
    eps = 32.0 * 2.0 ** -24 * mag
    z_lo = min(_corner_depths(b, cam)) - eps
    L = math.sqrt(float((R * R).sum())) * b.max_edge + 4.0 * eps
    if not z_lo > 1e-3:
        return math.inf
    ratio = L / z_lo
    if not ratio < 0.25:
        return math.inf
    ax = max(abs(cam.cx), abs(cam.W - cam.cx)) + 1.0
    ay = max(abs(cam.cy), abs(cam.H - cam.cy)) + 1.0
    return max((abs(cam.fx) + ax), (abs(cam.fy) + ay)) * ratio / (1.0 - ratio)


def huge_stage(b, cam):
    return not box_extent_bound(b, cam) <= MEDIUM - 4.0


def tpw_ladder(F, nviews=1):
    fine = F >= 32768
    min_waves, launch_views = (1024, max(1, nviews)) if fine else (2048, 1)
    tpw = 64
    while tpw > 1 and launch_views * F // tpw < min_waves:
        tpw >>= 1
    return tpw


def frag_groups(F, views, tpw, knobs=NO_KNOBS):
    if tpw != 64:
        return 1
    if knobs["groups"] >= 1:
        return knobs["groups"]
    return 4 if F >= 4000000 and views * -(-F // 256) >= 20480 else 1


def blocks(F, tpw, groups=1):
    return -(-(-(-F // (tpw * groups))) // 4)


def chunk(nblocks):
    return XCD_RUN if nblocks >= 64 else 0


def vote(verdicts):
    votes = sum(1 for v in verdicts if v)
    return 2 * votes >= len(verdicts) and votes > 0


def wants_wg_push(b, cam, knobs=NO_KNOBS):
    return knobs["wg_push"] != 0 if knobs["wg_push"] >= 0 else typical_edge_pixels(b, cam) >= 5.0


def wants_balance(b, cam, knobs=NO_KNOBS):
    return knobs["balance"] != 0 if knobs["balance"] >= 0 else depth_spread(b, cam) > 6.0


def wants_spread(b, cam, nviews, knobs=NO_KNOBS):
    if knobs["spread"] >= 0:
        return knobs["spread"] == 1
    if nviews > 1 or depth_spread(b, cam) > 6.0:
        return False
    return 10.5 <= typical_edge_pixels(b, cam) <= 19.0


def meshlet_tables(faces, V):
    """build_meshlets: every block of 256 consecutive faces uses at most 384 distinct vertices, every index inside [0, V)."""
    f = np.asarray(faces)
    if f.min() < 0 or f.max() >= V:
        return False
    return all(len(np.unique(f[k:k + MESHLET_TRIS])) <= MESHLET_MAX_VERTS for k in range(0, len(f), MESHLET_TRIS))


def keeps_face_order(vertices, faces):
    """spatial_order: below 4 096 faces always; else while the centroids of every 64 consecutive faces span, summed over the groups, at
    most 6 x 16 sampled edge lengths per group.  Returns (kept, spread / allowed)."""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces)
    F = len(f)
    if F < 4096:
        return True, 0.0
    c = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / np.float32(3)
    pad = (-F) % 64
    lo = np.concatenate([c, np.full((pad, 3), np.inf, np.float32)]).reshape(-1, 64, 3).min(1)
    hi = np.concatenate([c, np.full((pad, 3), -np.inf, np.float32)]).reshape(-1, 64, 3).max(1)
    before = float((hi.astype(np.float64) - lo).sum())
    s = np.arange(0, F, 16)
    edge = float(np.linalg.norm(v[f[s, 0]].astype(np.float64) - v[f[s, 1]], axis=1).mean())
    allowed = 6.0 * ((F + 63) // 64) * 16.0 * edge
    return before <= allowed, before / allowed


def mesh_info(mesh, texels=False):
    """What the dispatch knows of a mesh (cached on the mesh)."""
    key = "_info_%d" % texels
    if not hasattr(mesh, key):
        F, V = len(mesh.faces), len(mesh.vertices)
        setattr(mesh, key, types.SimpleNamespace(b=bounds(mesh.vertices, mesh.faces), F=F, V=V, texels=texels,
                                                 tables=meshlet_tables(mesh.faces, V), ordered=keeps_face_order(mesh.vertices, mesh.faces)[0]))
    return getattr(mesh, key)


def expected_render(info, cam, packed_option=True, depth=True, knobs=NO_KNOBS):
    """The report of one render() / fuse_view raster launch (render_into) plus the two formats."""
    b = info.b
    packed = packed_option and not info.texels and info.F <= PACKED_MAX_F
    spread = wants_spread(b, cam, 1, knobs)
    mode = (3 if spread else 1 if wants_wg_push(b, cam, knobs) else 0) | (4 if info.texels else 0) | (8 if packed else 0)
    tpw = SPREAD_TRIS if spread else tpw_ladder(info.F, 1)
    medium = (mode & 3) != 0 and wants_balance(b, cam, knobs)
    stages = 1 | (2 if medium else 0) | (4 if huge_stage(b, cam) else 0) | (8 if depth else 0) | (16 if packed else 0)
    return dict(kernel=1, mode=mode, views=1, tpw=tpw, groups=1, chunk=chunk(blocks(info.F, tpw)), stages=stages,
                record_format=16, fragment_format=8 if packed else 10)


def expected_group(info, cams, packed_option=True, meshlets_option=True, with_depth=False, compact=True, knobs=NO_KNOBS):
    """The report of one grouped raster launch (render_group_into) plus the raster path and the two formats."""
    b, n = info.b, len(cams)
    packed = packed_option and not info.texels and info.F <= PACKED_MAX_F
    spread = vote([wants_spread(b, cam, n, knobs) for cam in cams])
    push = vote([wants_wg_push(b, cam, knobs) for cam in cams])
    balance = vote([wants_balance(b, cam, knobs) for cam in cams])
    mode = (3 if spread else 1 if push else 0) | (4 if info.texels else 0)
    meshlets = (mode & 3) == 0 and info.tables and meshlets_option
    tpw = 64 if meshlets else SPREAD_TRIS if spread else tpw_ladder(info.F, n)
    groups = 1 if meshlets else frag_groups(info.F, n, tpw, knobs)
    medium = (mode & 3) != 0 and balance
    huge = any(huge_stage(b, cam) for cam in cams)
    stages = (0 if meshlets else 1) | (2 if medium else 0) | (4 if huge else 0) | (8 if with_depth else 0) | (16 if packed else 0)
    compact = compact and not with_depth and not info.texels and info.ordered and all(max(cam.W, cam.H) <= 8192 for cam in cams)
    return dict(kernel=3 if meshlets else 2, mode=mode | (8 if packed else 0), views=n, tpw=tpw, groups=groups,
                chunk=chunk(blocks(info.F, tpw, groups)), stages=stages, raster_path="meshlets" if meshlets else "vertex-stage",
                record_format=8 if compact else 16, fragment_format=8 if packed else 10)


def instances_of(report):
    """The names of the compiled instances a launch with this report consisted of."""
    mode, st = report["mode"], report["stages"]
    grp = "_group" if report["kernel"] in (2, 3) else ""
    tex, packed = bool(mode & 4), bool(st & 16)
    out = {"%s<%d>" % (KERNELS[report["kernel"]], mode)}
    if st & 2:
        out.add("k_raster_medium%s<%s>" % (grp, "true" if tex else "false, true" if packed else "false"))
    if st & 4:
        out.add("k_raster_huge" + grp)
    out.add("k_tile_resolve%s%s<%s>" % (grp, "_depth" if grp and st & 8 else "", "true" if packed else "false"))
    return out


MODES = (0, 1, 3, 4, 5, 7, 8, 9, 11)
_MEDIUM = ["k_raster_medium%s<%s>" % (g, a) for g in ("", "_group") for a in ("true", "false", "false, true")]
_RESOLVE = ["k_tile_resolve%s<%s>" % (g, p) for g in ("", "_group", "_group_depth") for p in ("true", "false")]
# what only a test hook reaches: no view of a group asks for spread waves (want_spread: nviews > 1), so their grouped instances need
# SMESH_RASTER_SPREAD=1.  (Two LAUNCH SHAPES are hook-only too, HOOK_ONLY_SHAPES: the medium stage behind a spread launch -- spread
# wants a depth spread <= 6, balance one > 6 -- and groups > 1 below four million faces.)
HOOK_ONLY = {"k_raster_frag_group<%d>" % m for m in (3, 7, 11)}
LIBRARY_INSTANCES = ({"k_raster_frag<%d>" % m for m in MODES} | {"k_raster_frag_group<%d>" % m for m in MODES}
                     | {"k_raster_frag_group_ml<%d>" % m for m in (0, 4, 8)} | set(_MEDIUM) | set(_RESOLVE)
                     | {"k_raster_huge", "k_raster_huge_group"}) - HOOK_ONLY
ALL_INSTANCES = LIBRARY_INSTANCES | HOOK_ONLY
HOOK_ONLY_SHAPES = ("spread + balance", "groups > 1")


# ---- boxes ---------------------------------------------------------------------------------------------------
def project(vertices, cam):
    """Vertex stage: Xc = R X + t in float32, left to right; u, v in double.  Returns (u, v, z_c)."""
    R, t, v = np.asarray(cam.R, np.float32), np.asarray(cam.t, np.float32), np.asarray(vertices, np.float32)
    pc = [((R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2]) + t[i] for i in range(3)]
    z = pc[2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return cam.fx * (pc[0].astype(np.float64) / z) + cam.cx, cam.fy * (pc[1].astype(np.float64) / z) + cam.cy, pc[2]


def box_classes(mesh, cam):
    """Per face: 0 off screen (or behind), 1 box within 8 x 8, 2 within 24 x 24 (a lane's own), 3 within 64 x 64 (a wave's), 4 larger,
    5 crossing the near plane.  Boxes: ceil(min - 0.5) .. floor(max - 0.5), clamped to the image."""
    u, s, z = project(mesh.vertices, cam)
    f = np.asarray(mesh.faces)
    front = (z > np.float32(1e-6))[f]
    allf, crossing = front.all(1), front.any(1) & ~front.all(1)
    uu, ss = np.where(allf[:, None], u[f], 0.0), np.where(allf[:, None], s[f], 0.0)
    x0, x1 = np.maximum(np.ceil(uu.min(1) - 0.5), 0), np.minimum(np.floor(uu.max(1) - 0.5), cam.W - 1)
    y0, y1 = np.maximum(np.ceil(ss.min(1) - 0.5), 0), np.minimum(np.floor(ss.max(1) - 0.5), cam.H - 1)
    bw, bh = (x1 - x0 + 1).astype(np.int64), (y1 - y0 + 1).astype(np.int64)
    side = np.maximum(bw, bh)
    cls = np.where(side <= 8, 1, np.where(side <= LANE_BOX, 2, np.where(side <= MEDIUM, 3, 4)))
    cls = np.where(allf & (bw > 0) & (bh > 0), cls, 0)
    return np.where(crossing, 5, cls), bw, bh


def class_counts(mesh, cam):
    return np.bincount(box_classes(mesh, cam)[0], minlength=6)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _mesh(vertices, faces):
    v, f = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return types.SimpleNamespace(vertices=v, faces=f)


@functools.lru_cache(maxsize=None)
def sheet(n, keep=None):
    """An n x n grid of unit cells in the plane z = 0 with 2 % depth noise, F = 2 n^2 (the first `keep` of them): faces in rows."""
    rng = np.random.default_rng(n)
    i, j = np.meshgrid(np.arange(n + 1, dtype=np.float64), np.arange(n + 1, dtype=np.float64), indexing="ij")
    v = np.stack([i - 0.5 * n, j - 0.5 * n, 0.02 * rng.uniform(-1, 1, i.shape)], -1).reshape(-1, 3)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (ii * (n + 1) + jj).reshape(-1)
    v10, v01, v11 = v00 + n + 1, v00 + 1, v00 + n + 2
    faces = np.stack([np.stack([v00, v10, v01], -1), np.stack([v10, v11, v01], -1)], 1).reshape(-1, 3)
    return _mesh(v, faces[:keep])


DISTANCE = 50.0


def head_on(mesh, edge, size=None, centre=(0.0, 0.0), aspect=1.0):
    """A camera DISTANCE above the plane z = 0 looking straight down, its focal length such that the typical edge (the restated
    estimate, on this very mesh) measures `edge` pixels.  `size`: (W, H), default the whole mesh plus four pixels each side."""
    b = mesh_info(mesh).b
    R = np.diag([1.0, -1.0, -1.0])
    t = np.array([0.0, 0.0, DISTANCE])
    f = edge * (DISTANCE - 0.5 * (b.lo[2] + b.hi[2])) / b.mean_edge
    f = float(np.float32(f))
    if size is None:
        size = (int(math.ceil((b.hi[0] - b.lo[0]) * f / DISTANCE)) + 8, int(math.ceil((b.hi[1] - b.lo[1]) * f * aspect / DISTANCE)) + 8)
    W, H = size
    return Cam(R, t, W, H, f, float(np.float32(f * aspect)), float(np.float32(0.5 * W + centre[0])), float(np.float32(0.5 * H + centre[1])))


ROOM_HALF = 5.0


@functools.lru_cache(maxsize=None)
def room(m):
    """A cube of side 10 around the origin, every wall a grid of m x m cells: F = 12 m^2, wall after wall."""
    g = np.linspace(-ROOM_HALF, ROOM_HALF, m + 1)
    a, c = np.meshgrid(g, g, indexing="ij")
    verts, faces = [], []
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    v00 = (ii * (m + 1) + jj).reshape(-1)
    v10, v01, v11 = v00 + m + 1, v00 + 1, v00 + m + 2
    cell = np.stack([np.stack([v00, v10, v01], -1), np.stack([v10, v11, v01], -1)], 1).reshape(-1, 3)
    for axis in range(3):
        for side in (-ROOM_HALF, ROOM_HALF):
            w = [a, c]
            w.insert(axis, np.full_like(a, side))
            faces.append(cell + len(verts) * (m + 1) ** 2)
            verts.append(np.stack(w, -1).reshape(-1, 3))
    return _mesh(np.concatenate(verts), np.concatenate(faces))


def looking_along_x(position, focal, size):
    """A camera at `position` that looks along +x (x_c = y, y_c = z, z_c = x)."""
    R = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    W, H = size
    return Cam(R, -R @ np.asarray(position, np.float64), W, H, float(focal), float(focal), 0.5 * W, 0.5 * H)


def inside(k=0, size=(300, 300), focal=30.0):
    """From inside the room, one unit behind its centre, with a wide lens: the box centre lies at depth 1, the typical edge beyond 5
    pixels; the side walls show from depth 1 on, where a cell of room(24) measures 44 pixels, and cross the camera plane."""
    return looking_along_x((-1.0, (0.3, -0.4, 0.1)[k % 3], (0.2, 0.5, -0.3)[k % 3]), focal, size)


def at_the_centre(size=(300, 300)):
    """From the room's very centre: the depth of the box centre is 0, so there is no estimate -- mode 0 although balance is set."""
    return looking_along_x((0.0, 0.0, 0.0), 30.0, size)


def outside(size=(160, 120)):
    """From thirty units away: depth spread 1.4, a wall cell under two pixels."""
    return looking_along_x((-30.0, 0.0, 0.0), 100.0, size)


# the decorations of `decorated()`: (class of box_classes, box in pixels, [(row, column of the cell whose first face is replaced)])
DECOR_N, DECOR_EDGE = 182, 2.5
RUN_30, RUN_5 = 64 * 519 + 1, 64 * 530 + 10         # first faces of the two runs of lane-box triangles
DECOR_SINGLES = {3: (40, [(96, 60), (97, 90), (98, 120)]), 4: (100, [(100, 91), (101, 80), (102, 100)]), 5: (6, [(104, 91), (105, 85), (106, 95)])}
DECOR_COUNTS = {2: 35, 3: 3, 4: 3, 5: 3}


@functools.lru_cache(maxsize=None)
def decorated():
    """sheet(182) less its last eleven faces (F = 66 237: 64 triangles per wave, a partial last wave and workgroup) at a typical edge
    of 2.5 pixels -- a cell measures about one pixel -- with triangles floating just above the faces they replace, so that the face
    order stays what the caller gave: thirty with boxes of 14 pixels in faces 33 217 .. 33 246 (one aligned wave: its lanes walk their
    own boxes in rounds), five in faces 33 930 .. 33 934 (fewer than kLaneBoxMin: the wave walks them), three of 40 pixels, three
    of 100 and three with a vertex behind the camera.  Returns (mesh, camera)."""
    n = DECOR_N
    base = sheet(n, 2 * n * n - 11)
    v, f = [np.array(base.vertices, np.float64)], np.array(base.faces)
    behind = DISTANCE + 0.5
    # the focal length the finished mesh will ask for: its box reaches the crossing triangles' far vertex (checked by the host test)
    focal = DECOR_EDGE * (DISTANCE - 0.5 * (behind - 0.02)) / mesh_info(base).b.mean_edge
    nv = len(base.vertices)

    def put(face, pixels, lift, crossing=False):
        nonlocal nv
        c = np.asarray(base.vertices, np.float64)[f[face]].mean(0)
        w = 0.5 * (pixels - 0.5) * (DISTANCE - lift) / focal
        tri = np.array([[c[0] - w, c[1] - w, lift], [c[0] + w, c[1] - w, lift], [c[0], c[1] + w, lift]])
        if crossing:
            tri[2, 2] = behind
        v.append(tri)
        f[face] = (nv, nv + 1, nv + 2)
        nv += 3

    for k in range(30):
        put(RUN_30 + k, 14, 0.05 + 0.004 * k)
    for k in range(5):
        put(RUN_5 + k, 14, 0.05 + 0.004 * k)
    for cls, (pixels, cells) in DECOR_SINGLES.items():
        for k, (i, j) in enumerate(cells):
            put(2 * (i * n + j), pixels, 0.1 * cls + 0.02 * k, crossing=cls == 5)
    mesh = _mesh(np.concatenate(v), f)
    return mesh, head_on(mesh, DECOR_EDGE)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# Face counts of the tpw ladder (one view): each leaves a partial last wave (but tpw 1) and a partial last workgroup of four waves.
#        F      sheet  tpw blocks
LADDER = {251: (12, 1, 63), 1797: (30, 1, 450), 4997: (50, 2, 625), 9797: (70, 4, 613), 19989: (100, 8, 625),
          39190: (140, 32, 307), 66237: (182, 64, 259)}


def ladder_sheet(F):
    return sheet(LADDER[F][0], F)


def _render_cases():
    """name -> (mesh, camera, texel renderer?, "packed_fragments", intended (mode, tpw, chunk, medium stage, huge stage))."""
    out = {}
    for F, (n, tpw, nb) in LADDER.items():
        m = ladder_sheet(F)
        out["ladder %d" % F] = (m, head_on(m, 2.5), False, 1, (8, tpw, 8 if nb >= 64 else 0, False, False))
    for F in (251, 39190):
        m = ladder_sheet(F)
        out["ladder %d unpacked" % F] = (m, head_on(m, 2.5), False, 0, (0, LADDER[F][1], 8 if LADDER[F][2] >= 64 else 0, False, False))
    big = ladder_sheet(66237)             # four full waves per workgroup at 64 triangles each; the image shows the sheet's middle
    out["edge 7 full waves"] = (big, head_on(big, 7.0, (448, 320), (30.0, -20.0)), False, 1, (9, 64, 8, False, False))
    out["edge 7 full waves unpacked"] = (big, head_on(big, 7.0, (448, 320), (30.0, -20.0)), False, 0, (1, 64, 8, False, False))
    mid = sheet(60, 7197)
    out["edge 14 spread"] = (mid, head_on(mid, 14.0, (500, 380)), False, 1, (11, 7, 8, False, False))
    out["edge 14 spread unpacked"] = (mid, head_on(mid, 14.0, (500, 380)), False, 0, (3, 7, 8, False, False))
    few = sheet(20, 797)
    out["edge 14 spread few blocks"] = (few, head_on(few, 14.0), False, 1, (11, 7, 0, False, False))
    coarse = sheet(16, 509)
    out["edge 30"] = (coarse, head_on(coarse, 30.0), False, 1, (9, 1, 8, False, True))     # (no proof at this size: an empty huge stage)
    dm, dc = decorated()
    out["decorated"] = (dm, dc, False, 1, (8, 64, 8, False, True))
    out["decorated unpacked"] = (dm, dc, False, 0, (0, 64, 8, False, True))
    r = room(24)
    out["room"] = (r, inside(), False, 1, (9, 2, 8, True, True))
    out["room unpacked"] = (r, inside(), False, 0, (1, 2, 8, True, True))
    out["room no estimate"] = (r, at_the_centre(), False, 1, (8, 2, 8, False, True))
    rb = room(60)
    out["room 32 per wave"] = (rb, inside(1, (360, 360), 60.0), False, 1, (9, 32, 8, True, True))
    tex = sheet(30, 1797)
    out["texels edge 2.5"] = (tex, head_on(tex, 2.5), True, 1, (4, 1, 8, False, False))
    out["texels edge 7"] = (tex, head_on(tex, 7.0), True, 1, (5, 1, 8, False, False))
    out["texels edge 14"] = (tex, head_on(tex, 14.0, (330, 250)), True, 1, (7, 7, 8, False, False))
    out["texels room"] = (r, inside(), True, 1, (5, 2, 8, True, True))
    return out


def _views(mesh, edges, sizes=None):
    """Head-on views of the given typical edges with mixed resolutions, the larger ones showing a part of the sheet."""
    sizes = sizes or [(96, 80), (120, 72), (88, 104), (64, 64)]
    return [head_on(mesh, e, sizes[k % len(sizes)], ((k % 3 - 1) * 5.0, (k % 2) * 4.0)) for k, e in enumerate(edges)]


SMALL, WIDE = 2.5, 7.0        # typical edges that vote against and for wg_push


def _group_cases():
    """name -> (mesh, cameras, texel renderer?, options {name: value}, route, intended (kernel, mode, tpw, medium stage), minority views).
    route: "plain" fuse_views, "depth" fuse_views(edge_gate=): the resolve writes depth planes."""
    g = sheet(39, 3037)
    big = ladder_sheet(39190)
    r = room(24)
    eight = [2.2, 2.4, 2.6, 2.8, 2.3, 2.5, 2.7, 2.9]
    out = {
        "three views": (g, _views(g, [2.3, 2.5, 2.8]), False, {}, "plain", (3, 8, 64, False), ()),
        "eight views meshlets": (g, _views(g, eight), False, {}, "plain", (3, 8, 64, False), ()),
        "eight views unpacked": (g, _views(g, eight), False, {"packed_fragments": 0}, "plain", (3, 0, 64, False), ()),
        "eight views vertex stage": (g, _views(g, eight), False, {"raster_meshlets": 0}, "plain", (2, 8, 1, False), ()),
        "eight views vertex stage unpacked": (g, _views(g, eight), False, {"raster_meshlets": 0, "packed_fragments": 0}, "plain", (2, 0, 1, False), ()),
        "four views full waves": (big, _views(big, [2.4, 2.5, 2.6, 2.7]), False, {"raster_meshlets": 0}, "plain", (2, 8, 64, False), ()),
        "push vote 1 of 4": (g, _views(g, [SMALL, WIDE, SMALL, SMALL]), False, {}, "plain", (3, 8, 64, False), (1,)),
        "push vote 2 of 4": (g, _views(g, [SMALL, WIDE, WIDE, SMALL]), False, {}, "plain", (2, 9, 1, False), (0, 3)),
        "push vote 3 of 4": (g, _views(g, [WIDE, WIDE, SMALL, WIDE]), False, {}, "plain", (2, 9, 1, False), (2,)),
        "push vote 3 of 4 unpacked": (g, _views(g, [WIDE, WIDE, SMALL, WIDE]), False, {"packed_fragments": 0}, "plain", (2, 1, 1, False), (2,)),
        "push vote 3 of 4 full waves": (big, _views(big, [WIDE, WIDE, SMALL, WIDE], [(160, 128), (144, 112)]), False, {}, "plain", (2, 9, 64, False), (2,)),
        "balance vote 2 of 3": (r, [inside(0), outside(), inside(1, (160, 176))], False, {}, "plain", (2, 9, 2, True), (1,)),
        "balance vote 2 of 3 unpacked": (r, [inside(0), outside(), inside(1, (160, 176))], False, {"packed_fragments": 0}, "plain", (2, 1, 2, True), (1,)),
        "depth planes": (g, _views(g, [2.3, 2.5, 2.8]), False, {}, "depth", (3, 8, 64, False), ()),
        "depth planes unpacked": (g, _views(g, [2.3, 2.5, 2.8]), False, {"packed_fragments": 0}, "depth", (3, 0, 64, False), ()),
        "texels meshlets": (g, _views(g, [2.3, 2.5, 2.8]), True, {}, "plain", (3, 4, 64, False), ()),
        "texels vertex stage": (g, _views(g, [2.3, 2.5, 2.8]), True, {"raster_meshlets": 0}, "plain", (2, 4, 1, False), ()),
        "texels push": (g, _views(g, [WIDE, WIDE, SMALL]), True, {}, "plain", (2, 5, 1, False), (2,)),
        "texels room": (r, [inside(0), outside(), inside(1, (160, 176))], True, {}, "plain", (2, 5, 2, True), (1,)),
    }
    return out


RENDER_CASES = _render_cases()
GROUP_CASES = _group_cases()

# ---- what only a hook reaches: one child process per knob setting --------------------------------------------------------------------
# knob -> (environment, restated knobs, [(kind, case name)]): the named cases of the tables above, run again under the knob.
HOOKS = {
    "spread": ({"SMESH_RASTER_SPREAD": "1"}, dict(NO_KNOBS, spread=1),
               [("group", "three views"), ("group", "eight views unpacked"), ("group", "texels meshlets")]),
    "spread balance": ({"SMESH_RASTER_SPREAD": "1", "SMESH_RASTER_BALANCE": "1"}, dict(NO_KNOBS, spread=1, balance=1),
                       [("render", "room"), ("render", "edge 14 spread unpacked"), ("group", "balance vote 2 of 3"), ("group", "texels room")]),
    "groups": ({"SMESH_RASTER_GROUPS": "4"}, dict(NO_KNOBS, groups=4),
               [("group", "four views full waves"), ("group", "push vote 3 of 4 full waves")]),
}
HOOK_INSTANCES = {"spread": {"k_raster_frag_group<11>", "k_raster_frag_group<3>", "k_raster_frag_group<7>"}}


def case_expectation(kind, name, knobs=NO_KNOBS):
    """The restated dispatch of a case of RENDER_CASES / GROUP_CASES."""
    if kind == "render":
        mesh, cam, texels, packed, _ = RENDER_CASES[name]
        return expected_render(mesh_info(mesh, texels), cam, bool(packed), True, knobs)
    mesh, cams, texels, options, route, _, _ = GROUP_CASES[name]
    return expected_group(mesh_info(mesh, texels), cams, bool(options.get("packed_fragments", 1)), bool(options.get("raster_meshlets", 1)),
                          route == "depth", True, knobs)
