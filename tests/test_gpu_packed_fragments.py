"""Packed fragment-queue entries (option "packed_fragments", semantic_meshes_amd/csrc/fragments.hpp) against the 10-byte format (a
64-bit key and a 16-bit pixel per fragment): one renderer, the same views, rendered and fused twice in one process -- option 0, then 1.

What must hold: the index and depth planes of render() and the raw accumulators of fuse_views are bit-equal, and each side's raster
launches really queued the format the scene is about ("last_fragment_format": 10 with the option off; 8 with it on, or 10 where the
renderer is outside the format's scope) -- comparing the 10-byte path with itself would prove nothing.

Class vectors as in tests/test_gpu_compact_records.py (its docstring gives the reason): arbitrary float32 where every box stays within
8 x 8 pixels, multiples of 1/64 with images_equal_weight = 0 where triangles are queued.  The scene helpers and the host-side box rule
are that module's.
"""
import numpy as np
import pytest

from test_gpu_compact_records import WIDE_SCALE, boxes, fine_grid, host_probs, queued, ring, stacked
from semantic_meshes_amd import data, synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def fragments_option(sm):
    """set(v) switches "packed_fragments"; the value found is restored."""
    before = sm._lib.get_option("packed_fragments")
    yield lambda v: sm._lib.set_option("packed_fragments", v)
    sm._lib.set_option("packed_fragments", before)


def duplicated(mesh):
    """Every face twice: the copies have the same depth everywhere, the lower id must win."""
    f = np.asarray(mesh.faces, np.int32)
    return data.Mesh(np.asarray(mesh.vertices, np.float32), np.concatenate([f, f]))


def one_side(sm, renderer, P, C, cams, dev, exact, expect, fuse=True):
    """(planes, raw) of the views with the option as it stands: render() of every camera -- index and depth plane as uint32 -- then
    fuse_views of all of them; the format of the last raster launch is asserted after each."""
    planes = []
    for cam in cams:
        idx, depth = renderer.render(cam, lazy=False)
        fmt = sm._lib.get_option("last_fragment_format")
        assert fmt == expect, ("render", fmt)
        planes.append((np.asarray(idx).view(np.uint32).copy(), np.asarray(depth).view(np.uint32).copy()))
    if not fuse:
        return planes, None
    agg = sm.fusion.MeshAggregator(P, C, "sum", 0.0 if exact else 0.5)
    agg.fuse_views(renderer, cams, dev)
    raw = agg.get_raw()
    fmt = sm._lib.get_option("last_fragment_format")
    assert fmt == expect, ("fuse_views", fmt)
    return planes, raw


def assert_equal_sides(a, b):
    (pa, ra), (pb, rb) = a, b
    for (ia, da), (ib, db) in zip(pa, pb):
        assert np.array_equal(ia, ib)
        assert np.array_equal(da, db)
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))


def both_formats(sm, set_option, renderer, P, C, cams, seed, expect=8, options=(0, 1)):
    """The sides of `options` in that order, each compared with the first; returns them.  Exact class vectors exactly where a triangle is
    queued in some view."""
    from semantic_meshes_amd.device import to_device
    exact = getattr(renderer, "_exact", False)
    dev = [to_device(p) for p in host_probs(cams, C, seed, exact=exact)]
    sides = []
    for opt in options:
        set_option(opt)
        sides.append(one_side(sm, renderer, P, C, cams, dev, exact, 10 if opt == 0 else expect))
    for s in sides[1:]:
        assert_equal_sides(sides[0], s)
    assert sides[0][1].any() and any((i != 0xFFFFFFFF).any() for i, _ in sides[0][0])
    return sides


def triangle_renderer(sm, mesh, cams):
    r = sm.render.triangles(mesh)
    r._exact = queued(mesh, cams) > 0
    return r


@pytest.mark.parametrize("n,C", [(8, 19), (3, 5)])
def test_small_boxes_across_the_tile_borders(sm, fragments_option, n, C):
    """(1) Boxes of at most 6 x 6 all over a 160 x 120 image: they straddle the tile borders at x = 32, 64, ... and y = 64, so lanes
    split their entries over up to four queues.  Arbitrary float32."""
    mesh, cams = fine_grid(), ring(n)
    r = triangle_renderer(sm, mesh, cams)
    assert not r._exact
    both_formats(sm, fragments_option, r, len(mesh.faces), C, cams, 41)


@pytest.mark.parametrize("scene", ["stacked", "duplicated"])
def test_contested_pixels(sm, fragments_option, scene):
    """(2) A: the grid and a copy 0.05 below it -- every pixel of the grid has a loser, lost() clears bits of the records.  B: every face
    twice, equal z at every pixel: the lower id wins in both formats."""
    base = fine_grid()
    mesh = stacked(base, 0.05) if scene == "stacked" else duplicated(base)
    cams = ring(8)
    P, half = len(mesh.faces), len(base.faces)
    r = triangle_renderer(sm, mesh, cams)
    assert not r._exact
    sides = both_formats(sm, fragments_option, r, P, 19, cams, 42)
    planes, raw = sides[1]
    if scene == "duplicated":
        for idx, _ in planes:
            assert (idx[idx != 0xFFFFFFFF] < half).all()               # never the copy
        assert not raw[half:].any()                                     # ... whose fragments all lost and were cleared
    else:
        assert sum(((idx >= half) & (idx < P)).sum() for idx, _ in planes) < sum((idx < half).sum() for idx, _ in planes)


def test_medium_and_lane_box_triangles(sm, fragments_option):
    """(3) The closer ring: boxes over 8 x 8 in the steeper views -- the lanes' rounds over sub-boxes and the cooperative walk, whose
    uncovered samples are null entries."""
    mesh, cams = fine_grid(), ring(8, WIDE_SCALE)
    over = 0
    for cam in cams:
        bw, bh, on = boxes(mesh, cam)
        over += int((((bw > 8) | (bh > 8)) & on).sum())
    print("(triangle, view) pairs with a box over 8 x 8:", over)
    assert over > 0
    r = triangle_renderer(sm, mesh, cams)
    assert r._exact
    both_formats(sm, fragments_option, r, len(mesh.faces), 19, cams, 43)


def test_image_not_a_multiple_of_the_tile(sm, fragments_option):
    """(4) 70 x 130: the last tile column is 6 pixels wide, the last tile row 2 pixels high."""
    mesh, cams = fine_grid(), ring(3, w=70, h=130)
    r = triangle_renderer(sm, mesh, cams)
    both_formats(sm, fragments_option, r, len(mesh.faces), 5, cams, 44)


@pytest.mark.parametrize("cap", ["1", "7"])
@pytest.mark.parametrize("scene", ["stacked", "duplicated"])
def test_queue_overflow_merges_the_key_image(sm, fragments_option, monkeypatch, scene, cap):
    """(5) Sub-queues of 1 and of 7 slots: most fragments go through the key image, whose keys the packed resolve converts as it seeds
    its slots; the resolve cannot name their losers and the fusion checks the masks against the index plane.  The same visible pixels
    as with queues that hold everything."""
    base = fine_grid()
    mesh = stacked(base, 0.05) if scene == "stacked" else duplicated(base)
    cams = ring(8)
    P = len(mesh.faces)
    monkeypatch.setenv("SMESH_FRAG_CAP", cap)
    r = triangle_renderer(sm, mesh, cams)
    overflow = both_formats(sm, fragments_option, r, P, 19, cams, 45)
    monkeypatch.delenv("SMESH_FRAG_CAP")
    r2 = triangle_renderer(sm, mesh, cams)
    plain = both_formats(sm, fragments_option, r2, P, 19, cams, 45)
    for (i0, d0), (i1, d1) in zip(overflow[1][0], plain[1][0]):
        assert np.array_equal(i0, i1) and np.array_equal(d0, d1)


BIG_A, BIG_B = 1024, 2048              # grid_mesh(1024, 2048): exactly 2^22 triangles


@pytest.fixture(scope="module")
def big_grid():
    mesh = synth.grid_mesh(BIG_A, BIG_B)
    assert len(mesh.faces) == 1 << 22
    return mesh


def corner_camera(size=64, focal=256.0, height=0.4):
    """Looks straight down at the grid's last corner (+x, +y: where the last face lies) from above all of the relief: a cell measures
    about 6 pixels, the last face covers some twenty."""
    s = 10.0 / BIG_A
    at = np.array([0.5 * BIG_A * s - 2.0 * s, 0.5 * BIG_B * s - 2.0 * s, 0.0])
    R, t = synth.look_at(at + np.array([0.0, 0.0, height]), at, up=(0.0, 1.0, 0.0))
    return data.Camera(R, t, np.asarray([size, size]), np.asarray([focal, focal], np.float64), np.asarray([size / 2.0, size / 2.0], np.float64))


def test_the_largest_id_that_fits(sm, fragments_option, big_grid):
    """(6a) 2^22 triangles: the format is 8, and id 2^22 - 1 -- all ones in the id field -- wins its pixels."""
    cams = [corner_camera()]
    last = (1 << 22) - 1
    r = sm.render.triangles(big_grid)
    sides = both_formats(sm, fragments_option, r, 1 << 22, 3, cams, 46)
    idx = sides[1][0][0][0]
    print("pixels of face %d: %d; background pixels: %d" % (last, int((idx == last).sum()), int((idx == 0xFFFFFFFF).sum())))
    assert (idx == last).any()
    assert (idx == 0xFFFFFFFF).any()                                   # beyond the corner: the background entry unpacks to -1 / +inf
    assert (sides[1][0][0][1][idx == 0xFFFFFFFF] == 0x7F800000).all()
    assert sides[1][1][last].any()


def test_one_face_beyond_the_limit(sm, fragments_option, big_grid):
    """(6b) The same mesh with one more face (a small triangle floating over the corner): 2^22 + 1 ids do not fit, the format is 10 with
    the option on, and the planes are those of the 2^22-face render wherever the new face does not show."""
    cam = corner_camera()
    s = 10.0 / BIG_A
    v, f = np.asarray(big_grid.vertices, np.float32), np.asarray(big_grid.faces, np.int32)
    V = len(v)
    cx, cy = 0.5 * BIG_A * s - 4.0 * s, 0.5 * BIG_B * s - 4.0 * s
    extra = np.array([[cx - s, cy - s, 0.05], [cx + s, cy - s, 0.05], [cx, cy + s, 0.05]], np.float32)
    more = data.Mesh(np.concatenate([v, extra]), np.concatenate([f, np.array([[V, V + 1, V + 2]], np.int32)]))
    P = (1 << 22) + 1
    r = sm.render.triangles(more)
    sides = both_formats(sm, fragments_option, r, P, 3, [cam], 47, expect=10)
    idx, depth = sides[1][0][0]
    assert (idx == P - 1).any()                                        # the new face shows
    fragments_option(1)
    (ref_idx, ref_depth), = one_side(sm, sm.render.triangles(big_grid), 1 << 22, 3, [cam], None, False, 8, fuse=False)[0]
    keep = idx != P - 1
    assert keep.any() and np.array_equal(idx[keep], ref_idx[keep]) and np.array_equal(depth[keep], ref_depth[keep])


def test_texel_renderers_keep_the_ten_byte_format(sm, fragments_option):
    """(7) A texel renderer's key holds a texel id: 10 bytes per fragment with the option on."""
    mesh, cams = fine_grid(), ring(3)
    r = sm.render.texels(mesh, cams, 1.5)
    r._exact = True
    P = r.getPrimitivesNum()
    assert P > len(mesh.faces)
    both_formats(sm, fragments_option, r, P, 5, cams, 48, expect=10)


def test_a_reordered_mesh_packs_the_callers_ids(sm, fragments_option):
    """(8) Faces handed over in shuffled order: the renderer re-orders them (F >= 4 096) and its entries hold the caller's ids from the
    prim_id table -- all below F, so the format is 8."""
    mesh = fine_grid(90, 24)                                           # 4 320 triangles
    perm = np.random.default_rng(6).permutation(len(mesh.faces))
    shuffled = data.Mesh(mesh.vertices, np.asarray(mesh.faces)[perm])
    cams = ring(3)
    r = sm.render.triangles(shuffled)
    r._exact = True
    sides = both_formats(sm, fragments_option, r, len(mesh.faces), 5, cams, 49)
    # the same mesh in its own order: pixel values map through the permutation
    fragments_option(1)
    straight = one_side(sm, sm.render.triangles(mesh), len(mesh.faces), 5, cams, None, True, 8, fuse=False)[0]
    for (idx, depth), (sidx, sdepth) in zip(sides[1][0], straight):
        hit = sidx != 0xFFFFFFFF
        assert np.array_equal(idx != 0xFFFFFFFF, hit) and np.array_equal(perm[idx[hit]], sidx[hit]) and np.array_equal(depth, sdepth)


def test_alternating_formats_on_one_renderer(sm, fragments_option):
    """(9) Option 0, 1, 0 on one renderer: a view slot's queues serve either format (the pixel array arrives with the first launch that
    needs it), and the third result is the first."""
    mesh, cams = stacked(fine_grid(), 0.05), ring(8, WIDE_SCALE)
    r = triangle_renderer(sm, mesh, cams)
    assert r._exact
    fragments_option(1)                                                # the slots' first launches are packed: no pixel array yet
    r.render(cams[0], lazy=False)
    assert sm._lib.get_option("last_fragment_format") == 8
    both_formats(sm, fragments_option, r, len(mesh.faces), 19, cams, 50, options=(0, 1, 0))
