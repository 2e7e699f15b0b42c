"""Grouped raster launches from meshlets (option "raster_meshlets", include/smesh_meshlets.h) against the same launches with the
vertex stage: one renderer, the same views, fused twice in one process -- option 0 (A) and option 1 (B).

What must hold: the raw accumulators are bit-equal, the index planes of the grouped launches are bit-equal, and the B side really
took the meshlet kernels (smesh_last_raster_path) -- comparing the vertex-stage path with itself would prove nothing.

Class vectors.  Scenes whose triangles all stay within 8 x 8 pixels use arbitrary float32 class vectors: every accumulator row
then sees one order of additions, and bit-equality also pins that order.  Scenes with queued triangles (near-plane crossings, boxes
over 8 x 8, texels) use class vectors that are multiples of 1/64 and images_equal_weight = 0 (every pixel weighs exactly 1): the
float atomics of queued triangles land in no fixed order in EITHER path -- two runs of the vertex-stage path differ in the last bit
of some sixty rows of scene (b) with ordinary inputs --, and with such values every partial sum is exact (below 2^18), so the sums
are bit-equal exactly when the two paths emit the same fragments: one fragment more or less on either side still changes them.
"""
import math

import numpy as np
import pytest

from helpers import BG, assert_fused_close, random_probs
from semantic_meshes_amd import data, label_images, synth

pytestmark = pytest.mark.gpu

GROUPS = [(3, 5), (8, 19)]        # (views per fuse_views call, classes): three views fill slots differently from a full group of eight


@pytest.fixture
def meshlets_option(sm):
    """set(v) switches "raster_meshlets"; the value found is restored."""
    before = sm._lib.get_option("raster_meshlets")
    yield lambda v: sm._lib.set_option("raster_meshlets", v)
    sm._lib.set_option("raster_meshlets", before)


def fine_grid(sm, a=100, b=15):
    """2 a b triangles of 2 - 4 pixels in the views below: the one-lane-per-triangle instances.  100 x 15: 3 000 = 11 * 256 + 184."""
    return synth.grid_mesh(a, b)


def ring(sm, n, W=160, H=120):
    return [synth.ring_camera(k, n, W, H) for k in range(n)]


def close_cameras(sm, mesh, n, W=160, H=120):
    """Cameras a few hundredths above the surface, looking along it and slightly down, from points well away from the mesh's centre (the
    mesh still measures a few pixels per edge at its centre): the triangles under and beside the eye cross the near plane in view."""
    v = np.asarray(mesh.vertices, np.float64)
    cams = []
    for k in range(n):
        p = v[(3 + k) * 16 + 9 + (k % 3)]                           # vertex (i, j) = (3 + k, 9 + k % 3) of the 100 x 15 grid: near its -x end
        eye = p + np.array([0.02, 0.03, 0.035 + 0.002 * k])
        heading = math.radians(-14.0 + 4.0 * k)
        target = eye + np.array([math.cos(heading), math.sin(heading), -0.30])
        R, t = synth.look_at(eye, target)
        f = 0.8 * W
        cams.append(data.Camera(R, t, np.asarray([W, H]), np.asarray([f, f], np.float64), np.asarray([W / 2.0, H / 2.0], np.float64)))
    return cams


def crossing_faces(mesh, cam):
    """Faces with vertices on both sides of the near plane, z_c computed like the vertex stage (float32)."""
    R, t = np.asarray(cam.rotation, np.float32), np.asarray(cam.translation, np.float32)
    v = np.asarray(mesh.vertices, np.float32)
    zc = ((R[2, 0] * v[:, 0] + R[2, 1] * v[:, 1]) + R[2, 2] * v[:, 2]) + t[2]
    front = (zc > np.float32(1e-6))[np.asarray(mesh.faces)]
    return np.nonzero(front.any(axis=1) & ~front.all(axis=1))[0]


def host_probs(sm, cams, C, seed, exact):
    rng = np.random.default_rng(seed)
    out = []
    for cam in cams:
        W, H = (int(x) for x in cam.resolution)
        p = random_probs(rng, W, H, C)
        if exact:
            p = (np.round(p * 64.0) / 64.0).astype(np.float32)
        out.append(p)
    return out


def fuse_both(sm, set_option, renderer, P, C, cams, probs, expect="meshlets", exact=False):
    """{0: raw, 1: raw} of fuse_views(cams) with the option off and on; the B side's path is asserted.  `exact`: `probs` are
    host_probs(exact=True) -- every pixel weighs 1 (see the module's docstring)."""
    from semantic_meshes_amd.device import to_device
    dev = [to_device(p) for p in probs]
    raws, aggs = {}, {}
    for opt in (0, 1):
        set_option(opt)
        agg = sm.fusion.MeshAggregator(P, C, "sum", 0.0 if exact else 0.5)
        agg.fuse_views(renderer, cams, dev)
        raws[opt] = agg.get_raw()
        path = sm._lib.last_raster_path()
        assert path == ("vertex-stage" if opt == 0 else expect), (opt, path)
        aggs[opt] = agg
    return raws, aggs


def index_planes(sm, renderer, P, cams):
    """The index planes of a GROUPED raster launch of `cams` as (n, W, H) uint16: label images with label(p) = p (P < 65535;
    background: 65535)."""
    lr = label_images.LabelRenderer(np.arange(P, dtype=np.int32), P, dtype=np.uint16, layout="WH")
    return np.asarray(lr.render_views(renderer, cams))


@pytest.mark.parametrize("n,C", GROUPS)
def test_tail_block_grid_bit_equal_and_oracle(sm, oracle, meshlets_option, n, C):
    """(a) F = 3 000 is no multiple of 256: the last workgroup of a view holds 184 triangles and 72 idle lanes.  Also against the oracle."""
    mesh, cams = fine_grid(sm), ring(sm, n)
    P = len(mesh.faces)
    assert P % 256 != 0
    r = sm.render.triangles(mesh)
    probs = host_probs(sm, cams, C, 11, exact=False)
    raws, aggs = fuse_both(sm, meshlets_option, r, P, C, cams, probs)
    assert np.array_equal(raws[0], raws[1])
    assert raws[1].any()
    o_r, o_a = oracle.OracleRenderer(mesh.vertices, mesh.faces), oracle.OracleAggregator(P, C)
    for cam, p in zip(cams, probs):
        o_a.add(o_r.render(cam)[0], p)
    assert_fused_close(aggs[1].get(), o_a.get())


def test_index_and_depth_planes_bit_equal(sm, oracle, meshlets_option):
    """The index planes the grouped launches leave, option off and on, and both against render(): the same planes.  Depth planes come
    from render() alone -- the single-view kernels, which the option does not touch -- and are compared across the option all the same."""
    mesh, cams = fine_grid(sm), ring(sm, 8)
    P = len(mesh.faces)
    r = sm.render.triangles(mesh)
    planes, depths = {}, {}
    for opt in (0, 1):
        meshlets_option(opt)
        planes[opt] = index_planes(sm, r, P, cams)
        assert sm._lib.last_raster_path() == ("meshlets" if opt else "vertex-stage")
        depths[opt] = [np.asarray(r.render(cam)[1]).view(np.uint32).copy() for cam in cams]
    assert np.array_equal(planes[0], planes[1])
    o_r = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    for k, cam in enumerate(cams):
        idx, depth = o_r.render(cam)
        assert np.array_equal(planes[1][k], np.where(idx == BG, 65535, idx).astype(np.uint16))
        assert np.array_equal(depths[0][k], depths[1][k]) and np.array_equal(depths[1][k], depth.view(np.uint32))
    assert (planes[1] != 65535).mean() > 0.05


@pytest.mark.parametrize("n,C", GROUPS)
def test_near_plane_crossings_recover_global_indices(sm, meshlets_option, n, C):
    """(b) Cameras close to the surface: some triangles cross the near plane, and those re-read their world-space vertices through
    the GLOBAL indices, which a meshlet lane has to look up in its block's id table."""
    mesh = fine_grid(sm)
    cams = close_cameras(sm, mesh, n)
    P = len(mesh.faces)
    r = sm.render.triangles(mesh)
    crossing = [crossing_faces(mesh, cam) for cam in cams]
    assert all(len(c) > 0 for c in crossing)
    raws, _ = fuse_both(sm, meshlets_option, r, P, C, cams, host_probs(sm, cams, C, 12, exact=True), exact=True)
    assert np.array_equal(raws[0], raws[1])
    planes = {}
    for opt in (0, 1):
        meshlets_option(opt)
        planes[opt] = index_planes(sm, r, P, cams)
        assert sm._lib.last_raster_path() == ("meshlets" if opt else "vertex-stage")
    assert np.array_equal(planes[0], planes[1])
    seen = sum(int(np.isin(planes[1][k], crossing[k]).sum()) for k in range(n))
    print("near-plane crossing faces per view %s, pixels showing one: %d" % ([len(c) for c in crossing], seen))
    assert seen > 0                                                    # a clipped triangle is actually on screen


@pytest.mark.parametrize("n,C", GROUPS)
def test_large_triangles_without_projected_vertices(sm, meshlets_option, n, C):
    """(c) A fine grid plus two triangles that span a third of the 224 x 168 image (boxes over 64 pixels: the tile workgroups of
    k_raster_huge_group shade them, with no array of projected vertices to read) and one of about a fifth (a whole wave walks it)."""
    mesh = fine_grid(sm, 100, 24)
    v, f = np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces, np.int32)
    V = len(v)
    extra_v = np.array([[-1.5, -1.15, 0.6], [1.4, -1.05, 0.7], [0.0, 1.35, 0.65],
                        [-0.3, -1.25, 0.9], [2.5, 0.2, 0.95], [0.2, 1.3, 1.0],
                        [-2.6, -0.5, 0.5], [-1.5, -0.6, 0.55], [-2.0, 0.45, 0.5]], np.float32)
    extra_f = np.array([[V, V + 1, V + 2], [V + 3, V + 4, V + 5], [V + 6, V + 7, V + 8]], np.int32)
    at = 1000                                                          # in the middle of a block, not at the end of the mesh
    mesh = data.Mesh(np.concatenate([v, extra_v]), np.concatenate([f[:at], extra_f, f[at:]]))
    P = len(mesh.faces)
    cams = ring(sm, n, 224, 168)
    r = sm.render.triangles(mesh)
    np.asarray(r.render(cams[0])[0])
    huge_stage, queues = r.render_stats(cams[0])
    print("view 0: huge stage needed %s, queue lengths %s" % (huge_stage, queues))
    assert huge_stage and queues[2] >= 2                               # (boxes over 64 pixels: the tile workgroups' queue)
    raws, _ = fuse_both(sm, meshlets_option, r, P, C, cams, host_probs(sm, cams, C, 13, exact=True), exact=True)
    assert np.array_equal(raws[0], raws[1])
    planes = {}
    for opt in (0, 1):
        meshlets_option(opt)
        planes[opt] = index_planes(sm, r, P, cams)
    assert np.array_equal(planes[0], planes[1])
    for big, least in ((at, 300), (at + 1, 300), (at + 2, 50)):       # all three are on screen
        assert (planes[1][0] == big).sum() > least, big


@pytest.mark.parametrize("n,C", GROUPS)
def test_shuffled_faces_keep_their_ids(sm, meshlets_option, n, C):
    """(d) Faces handed over in shuffled order: the renderer re-orders them (F >= 4 096) and the tables describe the RE-ORDERED faces,
    while the accumulator rows keep the caller's numbering (prim_id)."""
    mesh = fine_grid(sm, 90, 24)                                      # 4 320 triangles
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(mesh.faces))
    shuffled = data.Mesh(mesh.vertices, np.asarray(mesh.faces)[perm])
    P = len(mesh.faces)
    cams = ring(sm, n)
    probs = host_probs(sm, cams, C, 14, exact=True)
    r = sm.render.triangles(shuffled)
    raws, _ = fuse_both(sm, meshlets_option, r, P, C, cams, probs, exact=True)
    assert np.array_equal(raws[0], raws[1])
    # the same mesh in its own order: row perm[i] of that result is row i of this one
    straight, _ = fuse_both(sm, meshlets_option, sm.render.triangles(mesh), P, C, cams, probs, exact=True)
    assert np.array_equal(raws[1], straight[1][perm])


@pytest.mark.parametrize("n,C", GROUPS)
def test_texel_renderer_takes_the_texel_instance(sm, meshlets_option, n, C):
    """(e) A small texel renderer: the MODE 4 instance (the fragment's texel from its barycentric coordinates)."""
    mesh, cams = fine_grid(sm), ring(sm, n)
    r = sm.render.texels(mesh, cams, 1.5)
    P = r.getPrimitivesNum()
    assert P > len(mesh.faces)                                         # some triangles have more than one texel
    raws, _ = fuse_both(sm, meshlets_option, r, P, C, cams, host_probs(sm, cams, C, 15, exact=True), exact=True)
    assert np.array_equal(raws[0], raws[1])
    assert raws[1].any()


@pytest.mark.parametrize("n,C", GROUPS)
def test_a_soup_over_the_cap_keeps_the_vertex_stage(sm, meshlets_option, n, C):
    """(f) Every triangle with three vertices of its own: 768 distinct vertices per block, no tables -- the option changes nothing, and
    says so."""
    mesh = fine_grid(sm)
    f = np.asarray(mesh.faces)
    soup = data.Mesh(np.asarray(mesh.vertices)[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3))
    P = len(f)
    cams = ring(sm, n)
    probs = host_probs(sm, cams, C, 16, exact=False)
    raws, _ = fuse_both(sm, meshlets_option, sm.render.triangles(soup), P, C, cams, probs, expect="vertex-stage")
    assert np.array_equal(raws[0], raws[1])
    shared, _ = fuse_both(sm, meshlets_option, sm.render.triangles(mesh), P, C, cams, probs)
    assert np.array_equal(raws[1], shared[1])                          # the same triangles: the same sums from either path


def test_fuse_views_fuse_view_fuse_views_share_the_slots(sm, meshlets_option):
    """(g) fuse_views, fuse_view, fuse_views on one renderer: slot 0 serves a meshlet launch, then the single-view kernels (vertex
    stage, its own array of projected vertices), then a meshlet launch again; the queue counters of every view are emptied on the
    launch's own stream ahead of its raster kernel.  Twice over, so that both slot banks of the group pipeline come round again."""
    from semantic_meshes_amd.device import to_device
    mesh = fine_grid(sm)
    P, C = len(mesh.faces), 19
    cams = ring(sm, 8) + close_cameras(sm, mesh, 3) + ring(sm, 5)[1:4]
    probs = [to_device(p) for p in host_probs(sm, cams, C, 17, exact=True)]
    r = sm.render.triangles(mesh)
    raws = {}
    for opt in (0, 1):
        meshlets_option(opt)
        agg = sm.fusion.MeshAggregator(P, C, "sum", 0.0)               # (exact sums: the close cameras queue triangles)
        agg.defer = False                                              # fuse_view below is smesh_fuse_view, not a deferred group of one
        for _ in range(2):
            agg.fuse_views(r, cams[:8], probs[:8])
            agg.fuse_view(r, cams[8], probs[8])                        # (a close camera: queued triangles in slot 0's counters)
            agg.fuse_views(r, cams[8:11], probs[8:11])
            agg.fuse_view(r, cams[3], probs[3])
            agg.fuse_views(r, cams[11:], probs[11:])
        raws[opt] = agg.get_raw()
        assert sm._lib.last_raster_path() == ("meshlets" if opt else "vertex-stage")
    assert np.array_equal(raws[0], raws[1])
    assert raws[1].any()
