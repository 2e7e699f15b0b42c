"""Label and colour images of the fused mesh on the device (include/smesh_label_images.h, semantic_meshes_amd/label_images.py).

Every expected image is numpy on the definitions of the header: for index i, l = table[i] if 0 <= i < P else -1; the label is l and
the colour palette[l] where 0 <= l < K, else the don't-care label and colour.  Rendered views are compared on the ORACLE's index
images (the rasteriser is bit-exact against it).  All outputs are integers: all comparisons are array_equal."""
import ctypes

import numpy as np
import pytest

from helpers import BG, random_probs, small_scene

pytestmark = pytest.mark.gpu

P_TABLE = 1000
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 130), (67, 35), (64, 64), (128, 64), (65, 65), (257, 66)]
IDX_DTYPES = ("uint32", "int32", "uint64", "int64")
#          (classes, dtype, don't-care label, primitives)
CONFIGS = [(19, np.uint8, 255, P_TABLE),
           (255, np.uint8, 7, P_TABLE),          # a don't-care value that is also a class
           (300, np.uint16, 65535, P_TABLE),
           (19, np.uint8, 255, 0)]               # an empty table: every pixel is don't care
DC_COLOR = (9, 250, 77)


def make_palette(K):
    rng = np.random.default_rng(1000 + K)
    return rng.integers(0, 256, size=(K, 3)).astype(np.uint8)


def make_table(rng, P, K):
    """int32 [P]: classes, about 10 % of -1, K, K + 7; entries 0 .. 3 are a class, -1, K, K + 7."""
    t = rng.integers(0, K, size=P).astype(np.int32)
    odd = rng.random(P) < 0.1
    t = np.where(odd, rng.choice(np.array([-1, K, K + 7], np.int32), size=P), t).astype(np.int32)
    if P >= 4:
        t[:4] = [0, -1, K, K + 7]
    return t


def specials(dtype):
    """Index values of `dtype` that are no primitive of a table of P_TABLE entries: background, P, P + 7, the largest value, -1."""
    info = np.iinfo(dtype)
    vals = [0xFFFFFFFF if info.max >= 0xFFFFFFFF else int(info.max), P_TABLE, P_TABLE + 7, int(info.max)]
    if info.min < 0:
        vals.append(-1)
    return np.array(vals, dtype=dtype)


def make_indices(rng, W, H, dtype, rep):
    """(W,H) of `dtype`: primitives of [0, P_TABLE), about 10 % no primitive.  The first pixels are planted: primitive 0 (whose table
    entry is a class), a background value, P and P + 7 -- rotated by `rep`, so that images of fewer than four pixels show all four
    between them."""
    dt = np.dtype(dtype)
    idx = rng.integers(0, P_TABLE, size=W * H).astype(dt)
    sp = specials(dt)
    odd = rng.random(W * H) < 0.1
    idx = np.where(odd, rng.choice(sp, size=W * H), idx).astype(dt)
    plant = np.array([0, int(sp[0] if dt.kind == "u" else sp[-1]), P_TABLE, P_TABLE + 7], dtype=object).astype(dt)
    for k in range(min(4, W * H)):
        idx[k] = plant[(k + rep) % 4]
    return idx.reshape(W, H)


def widen(idx):
    idx = np.asarray(idx)
    return idx.astype(np.int64) if idx.dtype != np.uint64 else np.where(idx < 2 ** 62, idx, 2 ** 62).astype(np.int64)


def expected(idx, table, K, dtype, dc, palette, dc_color, layout):
    """(labels, colours) by the definition; (W,H[,3]) for layout "WH", (H,W[,3]) for "HW"."""
    wide = widen(idx)
    P = len(table)
    valid = (wide >= 0) & (wide < P)
    lab = np.where(valid, np.asarray(table, np.int64)[np.where(valid, wide, 0)], -1) if P else np.full(wide.shape, -1, np.int64)
    ok = (lab >= 0) & (lab < K)
    out = np.where(ok, lab, dc).astype(dtype)
    rgb = np.where(ok[..., None], palette[np.where(ok, lab, 0)], np.array(dc_color, np.uint8)).astype(np.uint8)
    if layout == "HW":
        return np.ascontiguousarray(out.T), np.ascontiguousarray(rgb.transpose(1, 0, 2))
    return out, rgb


def check(got, want, what):
    got = got.numpy() if hasattr(got, "numpy") else got
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


# ---- 1. render_image on synthetic index images ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_render_image(sm, shape):
    from semantic_meshes_amd.device import DeviceArray, to_device
    W, H = shape
    rng = np.random.default_rng(31 * W + H)
    reps = 4 if W * H < 4 else 1
    images = [(dt, make_indices(rng, W, H, dt, rep + k)) for k, dt in enumerate(IDX_DTYPES) for rep in range(reps)]
    # what this test's input really contains (with P = 1000)
    table19 = make_table(rng, P_TABLE, 19)
    wides = [widen(i) for _, i in images]
    assert any(((w >= 0) & (w < P_TABLE) & np.isin(w, np.flatnonzero((table19 >= 0) & (table19 < 19)))).any() for w in wides)   # covered, valid label
    assert any((i == BG).any() for dt, i in images if dt == "uint32") and any((w == -1).any() for w in wides)                  # background
    assert any((w >= P_TABLE).any() for w in wides)                                                                             # an index >= P
    for K, dtype, dc, P in CONFIGS:
        table = table19 if (K, P) == (19, P_TABLE) else make_table(rng, P, K)
        if P:
            assert ((table < 0) | (table >= K)).any() and {-1, K, K + 7} <= set(table.tolist())     # entries outside [0, K)
        palette = make_palette(K)
        for layout in ("HW", "WH"):
            lr = sm.fusion.LabelRenderer(table if layout == "HW" else to_device(table), K, palette=palette, dont_care_label=dc,
                                         dont_care_color=DC_COLOR, dtype=dtype, layout=layout)
            for dt, idx in images:
                want_l, want_c = expected(idx, table, K, dtype, dc, palette, DC_COLOR, layout)
                what = (shape, K, P, layout, dt)
                check(lr.render_image(idx), want_l, what)                                   # host in, numpy out
                check(lr.render_image_colors(idx), want_c, what)
                both = lr.render_image(to_device(idx), colors=True)                         # device in, numpy out, one pass
                check(both[0], want_l, what)
                check(both[1], want_c, what)
                dev = lr.render_image_device(idx, colors=True)                              # host in, device out
                assert isinstance(dev[0], DeviceArray) and isinstance(dev[1], DeviceArray)
                check(dev[0], want_l, what)
                check(dev[1], want_c, what)
                d_idx = to_device(idx)                                                      # device in, device out
                check(lr.render_image_device(d_idx), want_l, what)
                check(lr.render_image_colors_device(d_idx), want_c, what)
                lr.synchronize()
            # strided index images: an (H,W) array handed over as its transposed view, and every second column of a wider one
            for dt in ("uint32", "int64"):
                idx = next(i for d, i in images if d == dt)
                want_l, want_c = expected(idx, table, K, dtype, dc, palette, DC_COLOR, layout)
                as_hw = np.ascontiguousarray(idx.T)
                wide = np.zeros((W, 2 * H), idx.dtype)
                wide[:, ::2] = idx
                wide[:, 1::2] = 5                                                            # (what must not be read)
                for name, arg in (("host transposed", as_hw.T), ("device transposed", to_device(as_hw).T),
                                  ("host columns", wide[:, ::2]), ("device columns", DeviceArray_columns(to_device(wide)))):
                    what = (shape, K, P, layout, dt, name)
                    both = lr.render_image(arg, colors=True)
                    check(both[0], want_l, what)
                    check(both[1], want_c, what)
                    check(lr.render_image_device(arg), want_l, what)


def DeviceArray_columns(a):
    """Every second column of a dense (W, 2H) device array: (W,H) at element strides (2H, 2)."""
    from semantic_meshes_amd.device import DeviceArray
    W, H2 = a.shape
    return DeviceArray(a.ptr, (W, H2 // 2), a.dtype, a.device, (H2, 2), owner=a)


# ---- 2. render_views against the oracle's index images ----------------------------------------------------------------------------
K_VIEW = 19
N_VIEWS = (0, 1, 8, 9, 17)


@pytest.fixture(scope="module")
def view_scenes(sm, oracle):
    """{name: (renderer, [17 cameras], [their oracle index images], P)}: the small scene through the triangle renderer at 160 x 120
    and at 67 x 35, and through a texel renderer at 160 x 120.  Rendered once by the oracle; nothing here changes."""
    from semantic_meshes_amd import synth
    mesh, cams3 = small_scene()
    out = {}
    tri = sm.render.triangles(mesh)
    o_tri = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    for name, (W, H) in (("triangles 160x120", (160, 120)), ("triangles 67x35", (67, 35))):
        cams = [synth.ring_camera(k, 17, W, H) for k in range(17)]
        out[name] = (tri, cams, [o_tri.render(c)[0] for c in cams], len(mesh.faces))
    tex = sm.render.texels(mesh, cams3, 0.5)
    o_tex = oracle.OracleRenderer(mesh.vertices, mesh.faces, cams3, 0.5)
    cams = [synth.ring_camera(k, 17, 160, 120) for k in range(17)]
    assert tex.getPrimitivesNum() == o_tex.getPrimitivesNum() > len(mesh.faces)
    out["texels 160x120"] = (tex, cams, [o_tex.render(c)[0] for c in cams], tex.getPrimitivesNum())
    for _, _, idxs, P in out.values():
        for idx in idxs:
            assert (idx == BG).any() and (idx != BG).any() and idx[idx != BG].max() < P      # covered and background pixels
            idx.setflags(write=False)
    return out


def view_table(rng, idxs, P, K):
    """A table for rendered views: make_table, with a -1 planted on a primitive that view 0 shows."""
    table = make_table(rng, P, K)
    seen = np.unique(idxs[0][idxs[0] != BG])
    table[seen[len(seen) // 2]] = -1
    assert (table[seen] == -1).any() and ((table[seen] >= 0) & (table[seen] < K)).any()
    return table


@pytest.mark.parametrize("name", ["triangles 160x120", "triangles 67x35", "texels 160x120"])
def test_render_views(sm, view_scenes, name):
    from semantic_meshes_amd.device import DeviceArray, to_device
    renderer, cams, idxs, P = view_scenes[name]
    rng = np.random.default_rng(len(name))
    K = K_VIEW
    table, palette = view_table(rng, idxs, P, K), make_palette(K)
    W, H = cams[0].resolution
    hw = sm.fusion.LabelRenderer(to_device(table), K, palette=palette, dont_care_color=DC_COLOR)               # the defaults: uint8, 255, "HW"
    wh = sm.fusion.LabelRenderer(table, K, palette=palette, dont_care_color=DC_COLOR, layout="WH")
    want = {lay: [expected(i, table, K, np.uint8, 255, palette, DC_COLOR, lay) for i in idxs] for lay in ("HW", "WH")}
    for n in N_VIEWS:
        labels, colors = hw.render_views(renderer, cams[:n], colors=True)                     # both from one pass, on the host
        assert labels.shape == ((n, H, W) if n else (0, 0, 0)) and colors.shape == labels.shape + (3,)
        for v in range(n):
            check(labels[v], want["HW"][v][0], (name, n, v))
            check(colors[v], want["HW"][v][1], (name, n, v))
        dev = wh.render_views_device(renderer, cams[:n])                                      # labels only, left on the device
        assert isinstance(dev, DeviceArray) and dev.shape == ((n, W, H) if n else (0, 0, 0))
        got = dev.numpy()
        for v in range(n):
            check(got[v], want["WH"][v][0], (name, n, v, "WH"))
        rgb = wh.render_views_colors(renderer, cams[:n])                                      # colours only
        for v in range(n):
            check(rgb[v], want["WH"][v][1], (name, n, v, "WH colours"))
    check(hw.render_view(renderer, cams[3]), want["HW"][3][0], (name, "one view"))
    one = hw.render_view_device(renderer, cams[4], colors=True)
    check(one[0], want["HW"][4][0], (name, "one view, device"))
    check(one[1], want["HW"][4][1], (name, "one view, device"))
    check(hw.render_views_colors_device(renderer, cams[:9]).numpy()[8], want["HW"][8][1], (name, "colours, device"))


def test_render_views_of_two_resolutions_returns_a_list(sm, view_scenes):
    renderer, cams_a, idx_a, P = view_scenes["triangles 160x120"]
    _, cams_b, idx_b, _ = view_scenes["triangles 67x35"]
    rng = np.random.default_rng(17)
    K = K_VIEW
    table, palette = view_table(rng, idx_a, P, K), make_palette(K)
    order = [("a", 0), ("b", 1), ("a", 2), ("a", 3), ("b", 0), ("b", 5), ("a", 6), ("a", 7), ("b", 8), ("a", 9)]    # a group of eight and two more
    cams = [(cams_a if s == "a" else cams_b)[k] for s, k in order]
    idxs = [(idx_a if s == "a" else idx_b)[k] for s, k in order]
    for layout in ("HW", "WH"):
        lr = sm.fusion.LabelRenderer(table, K, palette=palette, dont_care_color=DC_COLOR, layout=layout)
        labels, colors = lr.render_views(renderer, cams, colors=True)
        dev = lr.render_views_device(renderer, cams)
        assert isinstance(labels, list) and isinstance(colors, list) and isinstance(dev, list) and len(labels) == len(cams)
        for v, idx in enumerate(idxs):
            want_l, want_c = expected(idx, table, K, np.uint8, 255, palette, DC_COLOR, layout)
            check(labels[v], want_l, (layout, v))
            check(colors[v], want_c, (layout, v))
            check(dev[v], want_l, (layout, v, "device"))


# ---- 3. agreement with the rest of the library ------------------------------------------------------------------------------------
def rule(rows, threshold):
    """The label rule of smesh_eval.h in numpy: float32, the row total in ascending class order."""
    rows = np.asarray(rows, np.float32)
    t = np.zeros(rows.shape[:-1], np.float32)
    for c in range(rows.shape[-1]):
        t = (t + rows[..., c]).astype(np.float32)
    lab = rows.argmax(axis=-1).astype(np.int32)
    lab[t < np.float32(threshold)] = -1
    return lab


def test_agreement_with_model_renderer_and_confusion_matrix(sm, view_scenes):
    from semantic_meshes_amd import synth
    renderer, _, _, P = view_scenes["triangles 160x120"]
    rng = np.random.default_rng(23)
    K, W, H = K_VIEW, 160, 120
    # three views from close by, which together leave part of the mesh unseen: rows below the threshold, labels of -1
    fuse_cams = [synth.ring_camera(k, 3, W, H, radius_scale=0.3) for k in range(3)]
    agg = sm.fusion.MeshAggregator(P, K)
    for cam in fuse_cams:
        agg.fuse_view(renderer, cam, random_probs(rng, W, H, K, zero_fraction=0.1))
    labels = agg.labels_device(0.9)
    host = labels.numpy()
    assert (host == -1).any() and (host >= 0).any()
    lr = sm.fusion.LabelRenderer(labels, K, layout="WH")
    mr = sm.fusion.ModelRenderer(agg)
    cams = [synth.ring_camera(k, 17, W, H) for k in (0, 5, 11)]
    got = lr.render_views(renderer, cams)
    cm = sm.fusion.ConfusionMatrix(K)
    for v, cam in enumerate(cams):
        idx = renderer.render_numpy(cam)[0]
        want = rule(mr.render(idx), 0.9)                      # (W,H,C) annotations, all zero where no primitive is: don't care
        assert (want == -1).any() and (want >= 0).any()
        check(got[v], np.where(want >= 0, want, 255).astype(np.uint8), v)
        gt = rng.integers(0, K + 1, size=(W, H)).astype(np.uint8)
        cm.reset()
        cm.add_image(idx, labels, gt)
        M = cm.get()
        hits = np.array([((got[v] == g) & (gt == g)).sum() for g in range(K)], np.uint64)
        assert hits.sum() > 0 and np.array_equal(np.diagonal(M[:, :K]), hits), v


# ---- 4. nothing else moves --------------------------------------------------------------------------------------------------------
def test_rendering_changes_neither_the_aggregator_nor_later_fusion(sm):
    from semantic_meshes_amd.device import to_device
    mesh, cams = small_scene(170, 81, 320, 240, views=3)      # (two- and three-pixel triangles: no float atomics, one order of additions)
    rng = np.random.default_rng(29)
    K, P = K_VIEW, len(mesh.faces)
    probs = [to_device(random_probs(rng, 320, 240, K)) for _ in cams]
    plain_renderer = sm.render.triangles(mesh)
    plain = sm.fusion.MeshAggregator(P, K)
    plain.fuse_views(plain_renderer, cams, probs)
    renderer = sm.render.triangles(mesh)
    agg = sm.fusion.MeshAggregator(P, K)
    agg.fuse_views(renderer, cams[:2], probs[:2])
    before_get, before_raw = agg.get(), agg.get_raw()
    lr = sm.fusion.LabelRenderer(agg.labels_device(0.9), K, palette=make_palette(K))
    images = lr.render_views(renderer, cams + cams + cams, colors=True)                       # nine views: two groups
    assert images[0].shape == (9, 240, 320) and (images[0] != 255).any()
    assert np.array_equal(agg.get().view(np.uint32), before_get.view(np.uint32))
    assert np.array_equal(agg.get_raw().view(np.uint32), before_raw.view(np.uint32))
    agg.fuse_views(renderer, cams[2:], probs[2:])                                             # ... the same renderer goes on fusing
    assert np.array_equal(agg.get_raw().view(np.uint32), plain.get_raw().view(np.uint32))


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(sm, view_scenes):
    from semantic_meshes_amd import _lib
    from semantic_meshes_amd.device import to_device
    renderer, cams, idxs, P = view_scenes["triangles 160x120"]
    rng = np.random.default_rng(37)
    K = K_VIEW
    W, H = cams[0].resolution
    table = make_table(rng, P, K)
    lib = _lib.lib()
    pods = (_lib.CameraPOD * 2)(cams[0]._pod, cams[1]._pod)
    idx = np.ascontiguousarray(idxs[0])
    strides = (ctypes.c_int64 * 2)

    def outputs(mem):
        """Two label and two colour images full of a sentinel, and their pointer arrays."""
        lab, rgb = np.full((2, H, W), 0xA5, np.uint8), np.full((2, H, W, 3), 0xA5, np.uint8)
        if mem == _lib.MEM_DEVICE:
            lab, rgb = to_device(lab), to_device(rgb)
            base_l, base_c = lab.ptr, rgb.ptr
        else:
            base_l, base_c = lab.ctypes.data, rgb.ctypes.data
        lp = (ctypes.c_void_p * 2)(base_l, base_l + W * H)
        cp = (ctypes.c_void_p * 2)(base_c, base_c + 3 * W * H)
        return lab, rgb, lp, cp

    def untouched(*arrays):
        _lib.synchronize(0)
        return all((np.asarray(a) == 0xA5).all() for a in arrays)

    plain = sm.fusion.LabelRenderer(table, K)                                   # no palette
    with_palette = sm.fusion.LabelRenderer(table, K, palette=make_palette(K))
    short = sm.fusion.LabelRenderer(table[:-1], K, palette=make_palette(K))    # a table whose P differs from the renderer's
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        lab, rgb, lp, cp = outputs(mem)
        for lay in (_lib.LAYOUT_HW, _lib.LAYOUT_WH):
            assert lib.smesh_label_renderer_render_views(short._handle, renderer._h, pods, 2, lay, lp, cp, mem) == _lib.ERR_INVALID
            assert b"primitives" in lib.smesh_last_error()
            # a colour request without a palette, at the C level
            assert lib.smesh_label_renderer_render_views(plain._handle, renderer._h, pods, 2, lay, lp, cp, mem) == _lib.ERR_INVALID
            assert b"palette" in lib.smesh_last_error()
            assert lib.smesh_label_renderer_render_image(plain._handle, idx.ctypes.data_as(ctypes.c_void_p), _lib.IDX_U32, None, _lib.MEM_HOST,
                                                         W, H, lay, lp[0], cp[0], mem) == _lib.ERR_INVALID
            # a negative stride
            for bad in ((-H, 1), (H, -1)):
                assert lib.smesh_label_renderer_render_image(with_palette._handle, idx.ctypes.data_as(ctypes.c_void_p), _lib.IDX_U32, strides(*bad),
                                                             _lib.MEM_HOST, W, H, lay, lp[0], cp[0], mem) == _lib.ERR_INVALID
                assert b"stride" in lib.smesh_last_error()
            # an unknown layout, no output at all
            assert lib.smesh_label_renderer_render_views(with_palette._handle, renderer._h, pods, 2, 2, lp, cp, mem) == _lib.ERR_INVALID
            assert lib.smesh_label_renderer_render_views(with_palette._handle, renderer._h, pods, 2, lay, None, None, mem) == _lib.ERR_INVALID
        assert untouched(lab, rgb), mem
    # the same through the Python layer
    with pytest.raises(ValueError):
        short.render_views(renderer, cams[:2])
    with pytest.raises(ValueError):
        short.render_views_device(renderer, [])                                 # (P is checked even without a view)
    with pytest.raises(ValueError):
        plain.render_views_colors(renderer, cams[:2])
    with pytest.raises(ValueError):
        with_palette.render_image(idx.astype(np.float32))
    with pytest.raises(ValueError):
        with_palette.render_image(idx.ravel())
    # ... and the renderers still work
    check(with_palette.render_view(renderer, cams[0]), expected(idxs[0], table, K, np.uint8, 255, make_palette(K), (0, 0, 0), "HW")[0], "after the errors")


# ---- 6. unsigned tables, and renderers that hand their planes over one at a time ----------------------------------------------------
def test_unsigned_and_wide_host_tables(sm):
    """A host table of any integer dtype: values that are no class (the dtype's maximum, 2^40, negative ones) are don't care."""
    rng = np.random.default_rng(41)
    K, W, H = 19, 67, 35
    idx = make_indices(rng, W, H, "uint32", 0)
    palette = make_palette(K)
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int64):
        info = np.iinfo(dt)
        table = rng.integers(0, K, size=P_TABLE).astype(dt)
        table[::7] = info.max
        table[1::7] = K
        table[2::7] = min(int(info.max), 2 ** 40)
        if info.min < 0:
            table[3::7] = -1
            table[4::7] = info.min
        as_int = np.where((table >= 0) & (table < K), table, 0).astype(np.int64) - ((table < 0) | (table >= K))
        assert (as_int == -1).any() and (as_int >= 0).any()
        lr = sm.fusion.LabelRenderer(table, K, palette=palette, dont_care_color=DC_COLOR)
        want_l, want_c = expected(idx, as_int, K, np.uint8, 255, palette, DC_COLOR, "HW")
        got = lr.render_image(idx, colors=True)
        check(got[0], want_l, dt)
        check(got[1], want_c, dt)


_LAUNCH_COUNT_SCRIPT = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import semantic_meshes_amd as sm
from semantic_meshes_amd import _lib, synth
from helpers import BG, small_scene
from test_gpu_label_images import expected, make_palette, make_table, DC_COLOR
want_launches = int(sys.argv[2])
mesh, _ = small_scene()
cams = [synth.ring_camera(k, 17, 160, 120) for k in range(9)]
renderer = sm.render.triangles(mesh)
K, P = 19, len(mesh.faces)
table, palette = make_table(np.random.default_rng(3), P, K), make_palette(K)
idxs = [renderer.render_numpy(c)[0] for c in cams]
assert all((i == BG).any() and (i != BG).any() for i in idxs)
lib = _lib.lib()
for layout in ("HW", "WH"):
    lr = sm.fusion.LabelRenderer(table, K, palette=palette, dont_care_color=DC_COLOR, layout=layout)
    for on_device in (False, True, False):
        _lib.check(lib.smesh_profile_enable(0, 1 << _lib.PROF_LABEL_IMAGES))
        _lib.check(lib.smesh_profile_reset(0))
        lab, rgb = (lr.render_views_device if on_device else lr.render_views)(renderer, cams, colors=True)
        _lib.synchronize(0)
        ms, n, launches, views = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(lib.smesh_profile_read_ex(0, _lib.PROF_LABEL_IMAGES, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(launches), ctypes.byref(views)))
        _lib.check(lib.smesh_profile_enable(0, 0))
        assert (launches.value, views.value) == (want_launches, 9), (launches.value, views.value)
        lab, rgb = np.asarray(lab), np.asarray(rgb)
        for v, idx in enumerate(idxs):
            want_l, want_c = expected(idx, table, K, np.uint8, 255, palette, DC_COLOR, layout)
            assert np.array_equal(lab[v], want_l) and np.array_equal(rgb[v], want_c), (layout, on_device, v)
print("ok")
"""


@pytest.mark.parametrize("raster,launches", [("", 2), ("direct", 9)], ids=["grouped", "direct"])
def test_launches_per_call_in_a_child_process(raster, launches):
    """Nine views are two launches of the image kernel (a group of eight and one more) where the rasteriser hands a group's planes
    over together, and nine -- one per view, same images -- with the direct rasteriser (SMESH_RASTER=direct), which hands them over
    one at a time in one buffer.  The environment is read when the library starts, hence the child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("SMESH_RASTER", None)
    if raster:
        env["SMESH_RASTER"] = raster
    done = subprocess.run([sys.executable, "-c", _LAUNCH_COUNT_SCRIPT, root, str(launches)], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stdout[-2000:] + done.stderr[-4000:]


def test_a_host_index_image_at_wide_strides_through_the_c_interface(sm):
    """Every 20th column of a wide host array, and a span that is mostly gaps: strides the Python layer would make dense first."""
    from semantic_meshes_amd import _lib
    rng = np.random.default_rng(43)
    K, W, H = 19, 67, 35
    table, palette = make_table(rng, P_TABLE, K), make_palette(K)
    lr = sm.fusion.LabelRenderer(table, K, palette=palette, dont_care_color=DC_COLOR)
    lib = _lib.lib()
    for dt, code in (("uint32", _lib.IDX_U32), ("int64", _lib.IDX_I64)):
        idx = make_indices(rng, W, H, dt, 0)
        for s0, s1 in ((20 * H, 20), (3000, 70)):
            wide = np.full(1 + (W - 1) * s0 + (H - 1) * s1, 5, idx.dtype)          # (5: what must not be read)
            view = np.lib.stride_tricks.as_strided(wide, (W, H), (s0 * wide.itemsize, s1 * wide.itemsize))
            view[...] = idx
            want_l, want_c = expected(idx, table, K, np.uint8, 255, palette, DC_COLOR, "HW")
            lab, rgb = np.full((H, W), 0xA5, np.uint8), np.full((H, W, 3), 0xA5, np.uint8)
            _lib.check(lib.smesh_label_renderer_render_image(lr._handle, wide.ctypes.data_as(ctypes.c_void_p), code, (ctypes.c_int64 * 2)(s0, s1),
                                                             _lib.MEM_HOST, W, H, _lib.LAYOUT_HW, lab.ctypes.data_as(ctypes.c_void_p),
                                                             rgb.ctypes.data_as(ctypes.c_void_p), _lib.MEM_HOST))
            check(lab, want_l, (dt, s0, s1))
            check(rgb, want_c, (dt, s0, s1))
    with pytest.raises(ValueError):
        _lib.check(lib.smesh_label_renderer_render_image(lr._handle, wide.ctypes.data_as(ctypes.c_void_p), code, (ctypes.c_int64 * 2)(1 << 40, 1),
                                                         _lib.MEM_HOST, W, H, _lib.LAYOUT_HW, lab.ctypes.data_as(ctypes.c_void_p), None, _lib.MEM_HOST))
