"""Label images that are colour images (include/smesh_label_colors.h), without a GPU: the restatement against numpy and against a
dictionary walk written out here, that the test inputs can tell the wrong rules from the right one, the header against the ctypes
table, the refusals of the C entry points that come before a device is needed, and the Python argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

import label_colors_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(rng, n=5, w=9, h=7, channels=3):
    pal = lc.make_palette(rng, 12)
    return pal, [lc.make_image(rng, w, h, pal[rng.permutation(12)[:5]], channels) for _ in range(n)]


@pytest.mark.parametrize("channels", [3, 4])
def test_unique_is_numpy_unique_over_rows(channels):
    rng = np.random.default_rng(channels)
    _, images = _images(rng, channels=channels)
    images.append(np.array([[[1, 2, 3, 9], [3, 2, 1, 8]], [[0, 0, 0, 7], [255, 255, 255, 6]]], np.uint8)[..., :channels])
    for im in images:
        want = np.unique(im.reshape(-1, channels)[:, :3], axis=0)
        np.testing.assert_array_equal(lc.unique(im), want)
        assert lc.unique(im).dtype == np.uint8
    for dt in (np.uint8, np.uint16):
        flat = rng.integers(0, np.iinfo(dt).max + 1, size=(11, 5)).astype(dt)
        np.testing.assert_array_equal(lc.unique(flat), np.unique(flat))
        assert lc.unique(flat).dtype == dt


def test_ascending_keys_are_lexicographic_rows():
    rows = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 255, 255], [255, 0, 0], [1, 2, 3], [3, 2, 1]], np.uint8)
    order = np.argsort(lc.key_rgb(rows))
    np.testing.assert_array_equal(rows[order], np.unique(rows, axis=0))
    np.testing.assert_array_equal(lc.colors_of(lc.key_rgb(rows)), rows)


def _dictionary_walk(images):
    """colorize_mesh.py --remap's bookkeeping, spelled out: np.unique over the rows of each image, a new row gets the next class."""
    d = {}
    out = []
    for im in images:
        ch = 1 if im.ndim == 2 else im.shape[2]
        rows = im.reshape(-1, ch)[:, :3] if ch > 1 else im.reshape(-1, 1)
        uniq, inv = np.unique(rows, axis=0, return_inverse=True)
        cls = []
        for row in uniq:
            row = tuple(row.tolist())
            if row not in d:
                d[row] = len(d)
            cls.append(d[row])
        out.append(np.array(cls)[inv.reshape(-1)].reshape(im.shape[:2]))
    return d, out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_remap_is_the_dictionary_walk(seed):
    """Sequences that bring colours in different orders: the same images forwards, backwards and shuffled give different dictionaries,
    each equal to the walk's."""
    rng = np.random.default_rng(seed)
    _, images = _images(rng, n=6)
    seen = []
    for order in (list(range(6)), list(range(5, -1, -1)), rng.permutation(6).tolist()):
        seq = [images[i] for i in order]
        d, masks = _dictionary_walk(seq)
        r = lc.Remap().update(seq)
        assert {tuple(lc.colors_of([k])[0].tolist()): c for k, c in r.classes.items()} == d
        for im, want in zip(seq, masks):
            np.testing.assert_array_equal(r.apply(im), want)
        seen.append(tuple(sorted(d.items())))
    assert len(set(seen)) > 1
    flat = [rng.integers(0, 300, size=(6, 4)).astype(np.uint16) for _ in range(3)]
    d, masks = _dictionary_walk(flat)
    r = lc.Remap().update(flat)
    assert {(k,): c for k, c in r.classes.items()} == d
    np.testing.assert_array_equal(r.apply(flat[2]), masks[2])


def test_the_inputs_can_show_the_wrong_rules():
    """Channels read as b, g, r and alpha taken into the key: both give other distinct colours and another plane on the inputs the
    GPU tests use."""
    rng = np.random.default_rng(3)
    pal = lc.make_palette(rng, 7)
    for channels in (3, 4):
        im = lc.make_image(rng, 13, 9, pal, channels)
        right = lc.prepare(im, 5, (20, 17), pal)
        assert (right < 5).any() and (right == 255).any()
        assert (lc.prepare(im, 5, (20, 17), pal, key=lc.key_bgr) != right).any()
        assert not np.array_equal(lc.unique_keys(im, lc.key_bgr), lc.unique_keys(im))
        if channels == 4:
            assert (lc.prepare(im, 5, (20, 17), pal, key=lc.key_with_alpha) != right).any()
            assert len(lc.unique_keys(im, lc.key_with_alpha)) > len(lc.unique_keys(im))
    pair = np.array([[[1, 2, 3]], [[3, 2, 1]]], np.uint8)
    np.testing.assert_array_equal(lc.unique_keys(pair, lc.key_bgr), lc.unique_keys(pair))      # (a symmetric pair cannot show b, g, r ...)
    assert (lc.prepare(pair, 2, None, pair[:, 0]) != lc.prepare(pair, 2, None, pair[:, 0], key=lc.key_bgr)).all()      # (... but its plane can)


def test_the_lookup_inputs_hold_the_off_by_one_cases():
    rng = np.random.default_rng(4)
    pal = lc.make_palette(rng, 7)
    keys = np.sort(lc.key_rgb(pal))
    got = set(lc.unique_keys(lc.make_image(rng, 130, 67, pal)).tolist())
    assert 0 in got and (1 << 24) - 1 in got and set(keys.tolist()) <= got
    assert any(int(k) - 1 in got for k in keys) and any(int(k) + 1 in got for k in keys)


def test_header_and_ctypes_table_agree():
    from semantic_meshes_amd import _lib
    text = open(os.path.join(ROOT, "include", "smesh_label_colors.h")).read()
    declared = sorted(set(re.findall(r"^int (smesh_\w+)\(", text, re.M)))
    assert declared == sorted(_lib.LABEL_COLORS_SIGNATURES)
    for name in declared:
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.LABEL_COLORS_SIGNATURES[name][1]), name
    assert int(re.search(r"#define SMESH_LABEL_COLORS_LDS_MAX (\d+)", text).group(1)) == _lib.LABEL_COLORS_LDS_MAX
    # each fusion entry point is its plain counterpart plus (w, h, channels, keys, classes, K)
    for name in ("smesh_fuse_views_labels", "smesh_fuse_view_labels", "smesh_aggregator_add_labels"):
        assert _lib.LABEL_COLORS_SIGNATURES[name + "_colors"][1][:-6] == _lib.EXT_SIGNATURES[name][1]
    # nothing of this went into the older headers
    for other in ("smesh.h", "smesh_labels.h", "smesh_label_prep.h", "smesh_eval.h"):
        assert "colors" not in open(os.path.join(ROOT, "include", other)).read()


def test_c_refusals_that_need_no_device():
    """Everything smesh_labels_prepare_colors and smesh_colors_unique refuse is refused before a device context is asked for."""
    from semantic_meshes_amd import _lib
    lib = _lib.lib()
    img = np.zeros((4, 3, 3), np.uint8)
    iptr = img.ctypes.data_as(ctypes.c_void_p)
    keys, cls = np.array([5, 9, 700], np.uint32), np.array([0, 1, 2], np.int32)
    host, u8, u16 = _lib.MEM_HOST, _lib.LBL_CODES["uint8"], _lib.LBL_CODES["uint16"]
    out = ctypes.c_void_p(64)      # never written: every call below is refused

    def prepare(ch=3, strides=None, mem=host, w=4, h=3, k=keys, c=cls, K=3, C=5, odt=u8, W=8, H=6):
        return lib.smesh_labels_prepare_colors(iptr, ch, strides, mem, w, h, None if k is None else k.ctypes.data_as(ctypes.c_void_p),
                                               None if c is None else c.ctypes.data_as(ctypes.c_void_p), K, C, out, odt, W, H, 0)

    for kw in (dict(ch=1), dict(ch=2), dict(ch=5), dict(ch=0), dict(strides=(ctypes.c_int64 * 3)(9, 3, -1)), dict(strides=(ctypes.c_int64 * 3)(-9, 3, 1)),
               dict(mem=2), dict(w=0), dict(h=0), dict(w=65537), dict(W=65537), dict(W=65536, H=8192), dict(K=0), dict(K=(1 << 24) + 1), dict(k=None),
               dict(c=None), dict(k=np.array([5, 5, 700], np.uint32)), dict(k=np.array([9, 5, 700], np.uint32)),
               dict(k=np.array([5, 9, 1 << 24], np.uint32)), dict(C=300), dict(C=0), dict(C=70000, odt=u16), dict(odt=5)):
        assert prepare(**kw) == _lib.ERR_INVALID, kw
        assert lib.smesh_last_error()
    ptrs = (ctypes.c_void_p * 1)(img.ctypes.data)
    counts, got = np.zeros(1, np.uint64), np.zeros(8, np.uint32)

    def unique(ch=3, dt=u8, strides=None, mem=host, w=4, h=3, cap=8, k=got, n=counts):
        return lib.smesh_colors_unique(ptrs, 1, ch, dt, strides, mem, w, h, None if k is None else k.ctypes.data_as(ctypes.c_void_p), cap,
                                       None if n is None else n.ctypes.data_as(ctypes.c_void_p), 0)

    for kw in (dict(ch=2), dict(ch=0), dict(ch=5), dict(dt=u16), dict(dt=_lib.LBL_CODES["int8"]), dict(ch=1, dt=_lib.LBL_CODES["int32"]),
               dict(strides=(ctypes.c_int64 * 3)(9, -3, 1)), dict(mem=7), dict(w=65537), dict(k=None), dict(n=None)):
        assert unique(**kw) == _lib.ERR_INVALID, kw
    assert counts[0] == 0 and not got.any()


def test_color_table_validation():
    from semantic_meshes_amd import fusion
    rows = np.array([[3, 2, 1], [1, 2, 3], [0, 0, 0]], np.uint8)
    t = fusion.ColorTable(rows)
    np.testing.assert_array_equal(t.keys, [0, 0x010203, 0x030201])
    np.testing.assert_array_equal(t.classes, [2, 1, 0])
    assert t.keys.dtype == np.uint32 and t.classes.dtype == np.int32 and len(t) == 3
    np.testing.assert_array_equal(t.colors, rows[[2, 1, 0]])
    t = fusion.ColorTable(rows, [7, -1, 2 ** 40])
    np.testing.assert_array_equal(t.classes, [-1, -1, 7])
    twice = np.array([[1, 2, 3], [9, 9, 9], [1, 2, 3]], np.uint8)
    t = fusion.ColorTable(twice, [4, 5, 4])
    np.testing.assert_array_equal(t.keys, [0x010203, 0x090909])
    np.testing.assert_array_equal(t.classes, [4, 5])
    with pytest.raises(ValueError, match="two different classes"):
        fusion.ColorTable(twice)
    for bad in (rows.astype(np.int32), rows[:, :2], rows.reshape(-1), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError):
            fusion.ColorTable(bad)
    for bad in ([0, 1], np.zeros(3, np.float32), np.zeros((3, 1), np.int32)):
        with pytest.raises(ValueError):
            fusion.ColorTable(rows, bad)
    lc_keys, lc_cls = lc.sort_table(rows, [7, 8, 9])
    t = fusion.ColorTable(rows, [7, 8, 9])
    np.testing.assert_array_equal(t.keys, lc_keys)
    np.testing.assert_array_equal(t.classes, lc_cls)


def test_python_argument_errors_need_no_device():
    import types
    from semantic_meshes_amd import fusion
    from semantic_meshes_amd.evaluation import ConfusionMatrix
    from test_label_prep_host import _bare_aggregator
    a = _bare_aggregator()
    W, H = 8, 6
    idx = np.zeros((W, H), np.uint32)
    img, flat = np.zeros((W, H, 3), np.uint8), np.zeros((W, H), np.uint8)
    pal = np.array([[0, 0, 0], [1, 1, 1]], np.uint8)
    cam = types.SimpleNamespace(resolution=(W, H), _pod=None)
    r = types.SimpleNamespace(device=0, _h=None)
    calls = {"add_labels": lambda m, **kw: a.add_labels(idx, m, **kw),
             "fuse_view_labels": lambda m, **kw: a.fuse_view_labels(r, cam, m, **kw),
             "fuse_views_labels": lambda m, **kw: a.fuse_views_labels(r, [cam], [m], **kw),
             "prepare_labels_device": lambda m, **kw: fusion.prepare_labels_device(m, 5, (W, H), **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="exclude each other"):
            call(img, palette=pal, label_map=np.arange(4))
        with pytest.raises(ValueError, match="colours must be"):
            call(img, palette=pal.astype(np.int32))
        with pytest.raises(ValueError, match="rank 3"):      # only a ColorRemap takes a 2-D mask
            call(flat, palette=pal)
        with pytest.raises(ValueError, match="colour image is"):
            call(np.zeros((W, H, 2), np.uint8), palette=pal)
        with pytest.raises(ValueError, match="colour image is"):
            call(img.astype(np.uint16), palette=fusion.ColorTable(pal))
        with pytest.raises(ValueError):      # a palette does not excuse a size mismatch
            call(np.zeros((4, 3, 3), np.uint8), palette=pal)
    cm = object.__new__(ConfusionMatrix)
    cm.classes, cm.device, cm._h, cm._keep = 5, 0, None, []
    with pytest.raises(ValueError, match="not a ColorRemap"):
        cm._prepared_gt(img, (W, H), None, None, "ground truth", fusion.ColorRemap())
    with pytest.raises(ValueError, match="exclude each other"):
        cm._prepared_gt(img, (W, H), None, np.arange(3), "ground truth", pal)
    with pytest.raises(ValueError, match="must have shape"):
        cm._prepared_gt(np.zeros((4, 3, 3), np.uint8), (W, H), None, None, "ground truth", pal)
    remap = fusion.ColorRemap()
    assert len(remap) == 0 and remap.color_to_class == {}
    np.testing.assert_array_equal(remap.class_to_color(3), np.zeros((3, 3), np.uint8))
