"""Label images that are colour images on the GPU (include/smesh_label_colors.h): `unique_colors` and `prepare_labels(palette=)`
against label_colors_ref, exact; every fusion entry point with `palette=` against the same call on the reference-prepared plane and
against the CPU oracle fed one_hot of it -- bit for bit where one lane owns a row --; the fallback routes, the round trip through
`LabelRenderer`, the growing `ColorRemap`, and ground truth with `gt_palette=`."""
import numpy as np
import pytest

import label_colors_ref as lc
import label_prep_ref as lp
import resize_ref as ref
from test_gpu_label_prep import NATIVE, H, W, bits, fine_scene, option
from test_labels_host import one_hot

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES + lp.EXTRA_SHAPES
_cache = {}


# ---- distinct colours ------------------------------------------------------------------------------------------------------------
def color_sets(rng, w, h):
    """name -> (w,h,3) image: the colour sets that can trip the bitmap and the list."""
    def of(rows):
        rows = np.asarray(rows, np.uint8)
        return rows[rng.integers(0, len(rows), size=(w, h))] if w * h >= 2 * len(rows) else np.resize(rows, (w, h, 3))
    sets = {"one": of([[9, 8, 7]]), "first and last bit": of([[0, 0, 0], [255, 255, 255]]), "mirrored": of([[1, 2, 3], [3, 2, 1]]),
            "one word": of([[0, 1, 0x20], [0, 1, 0x3F]]), "neighbouring words": of([[0, 1, 0x3F], [0, 1, 0x40]]),
            "random": rng.integers(0, 256, size=(w, h, 3)).astype(np.uint8)}
    if w * h >= 2:      # (of() deals round where the image is too small for a random draw to show every colour)
        for name in ("first and last bit", "mirrored", "one word", "neighbouring words"):
            assert len(lc.unique(sets[name])) == 2, name
    return sets


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (130, 67), (300, 150)], ids=lambda s: "%dx%d" % s)
def test_unique_colors_equals_the_restatement(sm, shape):
    w, h = shape
    rng = np.random.default_rng(w)
    images = []
    for name, rgb in color_sets(rng, w, h).items():
        images.append((name, rgb))
        rgba = np.concatenate([rgb, rng.integers(0, 256, size=(w, h, 1)).astype(np.uint8)], axis=2)
        images.append((name + " alpha", rgba))
    images.append(("uint8", rng.integers(0, 256, size=(w, h)).astype(np.uint8)))
    images.append(("uint16", rng.integers(0, 65536, size=(w, h)).astype(np.uint16)))
    images.append(("uint16 ends", np.resize(np.array([0, 65535, 31, 32], np.uint16), (w, h))))
    if (w, h) == (300, 150):      # every pixel another colour: 45 000 keys, more than the first request holds
        every = lc.colors_of(rng.permutation(np.unique(rng.integers(0, 1 << 24, size=2 * w * h)))[:w * h]).reshape(w, h, 3)
        assert len(lc.unique(every)) == w * h > 4096
        images.append(("all different", every))
    calls = 0
    for name, src in images:
        want = lc.unique(src)
        for device in (False, True):
            for layout, image in lc.layouts(src, device).items():
                got = sm.fusion.unique_colors(image)
                assert got.dtype == want.dtype and got.shape == want.shape, (name, layout, device, got.shape, want.shape)
                np.testing.assert_array_equal(got, want, err_msg="%s %s device=%s" % (name, layout, device))
                calls += 1
    print("    %d calls" % calls)


def test_unique_colors_of_a_batch(sm):
    """Eleven images in one smesh_colors_unique call (a group of eight and three), through ColorRemap.update."""
    rng = np.random.default_rng(11)
    pal = lc.make_palette(rng, 30)
    images = [lc.make_image(rng, 40, 30, pal[rng.permutation(30)[:4]], absent=0.0) for _ in range(11)]
    remap = sm.fusion.ColorRemap().update(images)
    want = lc.Remap().update(images)
    assert {(k >> 16, (k >> 8) & 255, k & 255): c for k, c in want.classes.items()} == remap.color_to_class
    assert len(remap) == len(want.classes) > 8


# ---- the plane -------------------------------------------------------------------------------------------------------------------
def tables(rng, C, lds_max):
    """name -> (colours (K,3), classes [K]): 1, 7 (with a class of -1 and one >= C), 256, lds_max and lds_max + 904 entries."""
    out = {}
    for K in (1, 7, 256, lds_max, lds_max + 904):
        cls = lp.make_map(rng, K, C).astype(np.int64)
        if K == 7:
            cls[:] = [2, -1, C, 0, C + 7, C - 1, 1]
        if K == 1:
            cls[:] = C - 1
        out[K] = (lc.make_palette(rng, K), cls)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_prepare_labels_with_a_palette_equals_the_restatement(sm, shape):
    """Tables in LDS and in global memory, colours in the table and absent from it (key - 1 and key + 1 of present keys, key 0 and key
    2^24 - 1: lc.make_image), 3 and 4 channels, every layout from the host and the device, a uint8 and a uint16 plane: the bytes of
    label_colors_ref.prepare, one launch of k_labels_prepare_colors a call and none of k_labels_prepare."""
    (w, h), size = shape
    lds_max = option(sm, "labels_colors_lds_max")
    assert lds_max == sm._lib.LABEL_COLORS_LDS_MAX
    rng = np.random.default_rng(1000 * w + h)
    calls = 0
    plain = option(sm, "labels_prepare_launches")
    for C in (5, 300):
        for K, (colors, cls) in tables(rng, C, lds_max).items():
            table = sm.fusion.ColorTable(colors, cls)
            assert len(table) == K
            for channels in (3, 4):
                src = lc.make_image(rng, w, h, colors, channels, absent=0.3)
                want = lc.prepare(src, C, size, colors, cls)
                assert want.dtype == (np.uint8 if C <= 255 else np.uint16)
                for device in (False, True):
                    for layout, image in lc.layouts(src, device).items():
                        before = option(sm, "labels_colors_launches")
                        out = sm.fusion.prepare_labels(image, C, size, "nearest", palette=table)
                        assert option(sm, "labels_colors_launches") - before == 1
                        calls += 1
                        np.testing.assert_array_equal(out, want, err_msg="K=%d ch=%d %s device=%s C=%d" % (K, channels, layout, device, C))
    assert option(sm, "labels_prepare_launches") == plain
    print("    %d calls" % calls)


def test_prepare_labels_palette_forms(sm):
    """A (K,3) array is class = row; a ColorRemap is updated by the call and takes a 2-D mask; the device result; no resize keyword."""
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(2)
    pal = lc.make_palette(rng, 6)
    img = lc.make_image(rng, 9, 4, pal)
    np.testing.assert_array_equal(sm.fusion.prepare_labels(img, 5, palette=pal), lc.prepare(img, 5, None, pal))
    d = sm.fusion.prepare_labels_device(to_device(img), 300, (18, 8), "nearest", palette=pal)
    assert d.shape == (18, 8) and d.dtype == np.uint16
    np.testing.assert_array_equal(d.numpy(), lc.prepare(img, 300, (18, 8), pal))
    with pytest.raises(ValueError, match='resize="nearest"'):
        sm.fusion.prepare_labels(img, 5, (18, 8), palette=pal)
    remap = sm.fusion.ColorRemap()
    want = lc.Remap().update([img])
    np.testing.assert_array_equal(sm.fusion.prepare_labels(img, 300, palette=remap), lp.narrow(want.apply(img), 300))
    assert len(remap) == len(want.classes)
    with pytest.raises(ValueError, match="more than the 5 classes"):
        sm.fusion.prepare_labels(img, 5, palette=remap)
    flat = rng.integers(0, 400, size=(9, 4)).astype(np.uint16)
    r1, w1 = sm.fusion.ColorRemap(), lc.Remap().update([flat])
    np.testing.assert_array_equal(sm.fusion.prepare_labels(flat, 300, palette=r1), lp.narrow(w1.apply(flat), 300))
    assert r1.color_to_class == {(k,): c for k, c in w1.classes.items()}
    np.testing.assert_array_equal(r1.class_to_color(40)[:3], [[k & 255] * 3 for k in sorted(w1.classes)[:3]])


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
def fusion_inputs(size, C, n):
    """n colour images of FUSION_SOURCES[size], their palette (classes with -1 and >= C among them) and the reference-prepared
    (160,120) planes; generated once per key and left unchanged."""
    key = (size, C, n)
    if key not in _cache:
        w, h = lp.FUSION_SOURCES[size]
        rng = np.random.default_rng(19 * w + 5 * C)
        K = 40
        colors, cls = lc.make_palette(rng, K), lp.make_map(rng, K, C).astype(np.int64)
        images = [lc.make_image(rng, w, h, colors, 3 + (i % 2), absent=0.05) for i in range(n)]
        planes = [lc.prepare(x, C, (W, H), colors, cls) for x in images]
        assert any((p < C).any() for p in planes) and any((p >= C).any() for p in planes)
        _cache[key] = (images, colors, cls, planes)
    return _cache[key]


def handed_over(images, how):
    if how == "host":
        return images
    return [lc.layouts(x, True)["dense" if how == "device" else "transposed"] for x in images]


FUSION_CASES = [(size, kind, C) for size in sorted(lp.FUSION_SOURCES) for kind in ("sum", "summax") for C in (5, 19, 300)]


@pytest.mark.parametrize("size,kind,C", FUSION_CASES)
def test_fuse_views_labels_with_a_palette_bit_exact(sm, oracle, size, kind, C):
    """fuse_views_labels(palette=) on 11 views against the same call on the reference-prepared planes and against the oracle fed
    their one_hot: raw accumulators equal in bits.  Weights, image_equal_weight and the memory of the images are dealt round.  The
    images alternate between 3 and 4 channels, so the list of 11 is a mixed one and is fused view by view; every second image has
    three channels, and those six go to the library as one batch (test_color_remap_discovers_the_palette sends 11 as 8 + 3)."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    i = FUSION_CASES.index((size, kind, C))
    with_weights, iew, how = bool(i % 2), (0.0, 0.5, 1.0)[i % 3], ("host", "device", "transposed")[(i // 2) % 3]
    images, colors, cls, planes = fusion_inputs(size, C, len(cams))
    table = sm.fusion.ColorTable(colors, cls)
    rng = np.random.default_rng(9)
    weights = [rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) for _ in cams] if with_weights else None
    wts = weights if how == "host" or weights is None else [to_device(x) for x in weights]
    r = sm.render.triangles(mesh)
    oagg = oracle.OracleAggregator(P, C, kind, iew)
    for k in range(len(cams)):
        oagg.add(oidx[k], one_hot(planes[k], C), None if weights is None else weights[k])
    want = bits(oagg.get_raw())
    assert want.any()
    for pick in (slice(None), slice(0, None, 2)):      # mixed channel counts: view by view; one channel count: groups of eight
        sub = lambda xs: None if xs is None else xs[pick]      # noqa: E731
        agg, twin = sm.fusion.MeshAggregator(P, C, kind, iew), sm.fusion.MeshAggregator(P, C, kind, iew)
        before, plain = option(sm, "labels_colors_launches"), option(sm, "labels_prepare_launches")
        agg.fuse_views_labels(r, cams[pick], handed_over(images[pick], how), sub(wts), resize="nearest", palette=table)
        assert sm._lib.last_fuse_kernel() == NATIVE
        assert option(sm, "labels_colors_launches") - before == len(cams[pick]) and option(sm, "labels_prepare_launches") == plain
        twin.fuse_views_labels(r, cams[pick], planes[pick], sub(weights))
        np.testing.assert_array_equal(bits(agg.get_raw()), bits(twin.get_raw()))
        if pick == slice(None):
            np.testing.assert_array_equal(bits(agg.get_raw()), want)
            np.testing.assert_array_equal(bits(agg.get()), bits(oagg.get()))


@pytest.mark.parametrize("C", [19, 300])
def test_per_view_forms_with_a_palette(sm, oracle, C):
    """add_labels and fuse_view_labels with `palette=` between deferred plain calls: the deferred views are handed over first, and the
    bits are the oracle's for the same order."""
    from semantic_meshes_amd.device import to_device
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    images, colors, cls, planes = fusion_inputs("0.4", C, 11)
    table = sm.fusion.ColorTable(colors, cls)
    r = sm.render.triangles(mesh)
    a = sm.fusion.MeshAggregator(P, C, "sum", 0.5)
    pending = []
    for k in range(7):
        if k in (2, 5):
            a.add_labels(r.render(cams[k])[0], images[k], resize="nearest", palette=table)
        elif k == 3:
            a.fuse_view_labels(r, cams[k], lc.layouts(images[k], True)["transposed"], resize="nearest", palette=table)
        else:
            a.add_labels(r.render(cams[k])[0], to_device(planes[k]))
        pending.append(len(a._pending))
    assert max(pending) > 0 and pending[2] == pending[3] == pending[5] == 0
    oagg = oracle.OracleAggregator(P, C, "sum", 0.5)
    for k in range(7):
        oagg.add(oidx[k], one_hot(planes[k], C))
    np.testing.assert_array_equal(bits(a.get_raw()), bits(oagg.get_raw()))


def test_fallback_routes_with_a_palette(sm, oracle):
    """Mul, a texel renderer and a foreign index image: with `palette=` the result is, in bits, that of the plain call on the
    reference-prepared plane, and the same kernel ran."""
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    cams = cams[:3]
    C = 19
    images, colors, cls, planes = fusion_inputs("0.37", C, 11)
    table = sm.fusion.ColorTable(colors, cls)
    r = sm.render.triangles(mesh)
    rt = sm.render.texels(mesh, cams, 0.05)

    def twin(renderer, prims, kind, foreign):
        a, b = sm.fusion.MeshAggregator(prims, C, kind), sm.fusion.MeshAggregator(prims, C, kind)
        kernels = []
        for k, cam in enumerate(cams):
            if foreign:
                idx = np.asarray(renderer.render(cam)[0]).copy()
                a.add_labels(idx, images[k], resize="nearest", palette=table)
                kernels.append(sm._lib.last_fuse_kernel())
                b.add_labels(idx, planes[k])
            else:
                a.fuse_view_labels(renderer, cam, images[k], resize="nearest", palette=table)
                kernels.append(sm._lib.last_fuse_kernel())
                b.fuse_view_labels(renderer, cam, planes[k])
            kernels.append(sm._lib.last_fuse_kernel())
        assert kernels[0::2] == kernels[1::2] and NATIVE not in kernels, kernels
        ra, rb = bits(a.get_raw()), bits(b.get_raw())
        assert rb.any()
        np.testing.assert_array_equal(ra, rb)

    twin(r, P, "mul", False)
    twin(rt, rt.getPrimitivesNum(), "sum", False)
    twin(r, P, "sum", True)


def test_round_trip_through_the_label_renderer(sm, oracle):
    """LabelRenderer(labels, palette=P) renders the fused mesh into colour images; fed back through fuse_views_labels(palette=P) they
    give the accumulators of fusing the label images themselves, bit for bit (the don't-care colour is in no palette row)."""
    from semantic_meshes_amd.device import DeviceArray
    from semantic_meshes_amd.label_images import LabelRenderer
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    C = 19
    rng = np.random.default_rng(6)
    palette = lc.make_palette(rng, C)      # (lc.make_palette leaves key 0 out: black stays the don't-care colour)
    labels = rng.integers(-1, C, size=P).astype(np.int32)
    r = sm.render.triangles(mesh)
    lr = LabelRenderer(labels, C, palette=palette)
    lab, col = lr.render_views_device(r, cams, colors=True)
    n = len(cams)
    assert col.shape == (n, H, W, 3) and lab.shape == (n, H, W)
    col_views = [DeviceArray(col.ptr + k * H * W * 3, (W, H, 3), np.uint8, col.device, (3, 3 * W, 1), owner=col) for k in range(n)]
    lab_views = [DeviceArray(lab.ptr + k * H * W, (W, H), np.uint8, lab.device, (1, W), owner=lab) for k in range(n)]
    a, b = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    a.fuse_views_labels(r, cams, col_views, palette=palette)
    b.fuse_views_labels(r, cams, lab_views)
    assert bits(b.get_raw()).any()
    np.testing.assert_array_equal(bits(a.get_raw()), bits(b.get_raw()))


# ---- the growing palette ---------------------------------------------------------------------------------------------------------
def remap_images():
    """11 full-size images: image k holds colours k .. k + 3 of a 14-colour palette sorted by DESCENDING key, laid out in that order
    along x -- so inside an image the colours appear in descending key order, and new colours first appear in different images."""
    if "remap" not in _cache:
        rng = np.random.default_rng(21)
        pal = lc.make_palette(rng, 14)
        pal = pal[np.argsort(-lc.key_rgb(pal))]
        images = []
        for k in range(11):
            band = (np.arange(W) * 4 // W)[:, None] + np.zeros((1, H), np.int64)
            noise = rng.random((W, H)) < 0.2
            band[noise] = rng.integers(0, 4, size=int(noise.sum()))
            band[0, 0], band[W - 1, H - 1] = 0, 3
            images.append(np.ascontiguousarray(pal[k + band]))
        _cache["remap"] = images
    return _cache["remap"]


def test_color_remap_discovers_the_palette(sm, oracle):
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    images = remap_images()
    assert len(images) == len(cams) == 11
    want = lc.Remap().update(images)
    K = len(want.classes)
    assert K == 14
    # colours arrive in descending key order inside an image: pixel order and key order disagree
    first = lc.keys_of(images[0])
    assert first[0, 0] > first[-1, -1] and want.classes[int(first[-1, -1])] == 0
    masks = [lp.narrow(want.apply(x), K) for x in images]
    r = sm.render.triangles(mesh)
    dev = [lc.layouts(x, True)["transposed"] for x in images]
    remap = sm.fusion.ColorRemap()
    a = sm.fusion.MeshAggregator(P, K)
    a.fuse_views_labels(r, cams, dev, palette=remap)
    assert sm._lib.last_fuse_kernel() == NATIVE
    assert remap.color_to_class == {tuple(lc.colors_of([k])[0].tolist()): c for k, c in want.classes.items()}
    assert len(remap) == K
    back = remap.class_to_color(K + 2)
    for k, c in want.classes.items():
        np.testing.assert_array_equal(back[c], lc.colors_of([k])[0])
    assert not back[K:].any()
    loop_remap = sm.fusion.ColorRemap()
    b = sm.fusion.MeshAggregator(P, K)
    for cam, x in zip(cams, images):
        b.fuse_view_labels(r, cam, x, palette=loop_remap)
    c = sm.fusion.MeshAggregator(P, K)
    c.fuse_views_labels(r, cams, masks)
    ra = bits(a.get_raw())
    assert ra.any()
    np.testing.assert_array_equal(ra, bits(b.get_raw()))
    np.testing.assert_array_equal(ra, bits(c.get_raw()))
    assert loop_remap.color_to_class == remap.color_to_class
    # one class too few: refused before anything is fused; the remap keeps what it has seen
    small = sm.fusion.MeshAggregator(P, K - 1)
    small.fuse_views_labels(r, cams[:2], masks[:2])
    before = bits(small.get_raw()).copy()
    assert before.any()
    fresh = sm.fusion.ColorRemap()
    with pytest.raises(ValueError, match="more than the %d classes" % (K - 1)):
        small.fuse_views_labels(r, cams, dev, palette=fresh)
    np.testing.assert_array_equal(bits(small.get_raw()), before)
    assert len(fresh) == K
    # mixed channel counts
    flat = np.zeros((W, H), np.uint8)
    with pytest.raises(ValueError, match="one channel count"):
        sm.fusion.ColorRemap().update([images[0], flat])
    with pytest.raises(ValueError, match="one channel count"):
        a.fuse_view_labels(r, cams[0], flat, palette=remap)
    with pytest.raises(ValueError, match="one channel count"):
        sm.fusion.ColorRemap().update(flat).update(images[0])
    # 2-D masks: key = value
    rng = np.random.default_rng(8)
    flats = [rng.choice(np.array([200, 7, 90, 31, 255, 0], np.uint8)[k % 3:k % 3 + 4], size=(W, H)) for k in range(3)]
    fw = lc.Remap().update(flats)
    d, e = sm.fusion.MeshAggregator(P, 6), sm.fusion.MeshAggregator(P, 6)
    fr = sm.fusion.ColorRemap()
    d.fuse_views_labels(r, cams[:3], flats, palette=fr)
    e.fuse_views_labels(r, cams[:3], [lp.narrow(fw.apply(x), 6) for x in flats])
    assert fr.color_to_class == {(k,): c for k, c in fw.classes.items()}
    np.testing.assert_array_equal(bits(d.get_raw()), bits(e.get_raw()))


# ---- ground truth ----------------------------------------------------------------------------------------------------------------
def test_ground_truth_with_a_palette(sm, oracle):
    from semantic_meshes_amd.device import to_device
    from semantic_meshes_amd.evaluation import ConfusionMatrix
    mesh, cams, P, oidx = fine_scene(sm, oracle)
    cams = cams[:3]
    C = 19
    images, colors, cls, planes = fusion_inputs("0.37", C, 11)
    table = sm.fusion.ColorTable(colors, cls)
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, C, size=P).astype(np.int32)
    r = sm.render.triangles(mesh)

    def pair(with_keyword, plain):
        a, b = ConfusionMatrix(C), ConfusionMatrix(C)
        with_keyword(a)
        plain(b)
        Ma, Mb = a.get(), b.get()
        assert Mb.sum() > 0 and b.ignored > 0
        np.testing.assert_array_equal(Ma, Mb)
        assert a.ignored == b.ignored

    for imgs in (images[:3], [to_device(x) for x in images[:3]]):
        pair(lambda cm: cm.add_views(r, cams, labels, imgs, gt_resize="nearest", gt_palette=table), lambda cm: cm.add_views(r, cams, labels, planes[:3]))
    pair(lambda cm: cm.add_view(r, cams[1], labels, images[1], gt_resize="nearest", gt_palette=table), lambda cm: cm.add_view(r, cams[1], labels, planes[1]))
    idx = np.asarray(r.render(cams[0])[0]).copy()
    pair(lambda cm: cm.add_image(idx, labels, images[0], gt_resize="nearest", gt_palette=table), lambda cm: cm.add_image(idx, labels, planes[0]))
    # without gt_resize: a full-size colour image, a (K,3) array as the palette (class = row)
    pal = lc.make_palette(rng, C + 2)
    full = lc.make_image(rng, W, H, pal, 4)
    plane = lc.prepare(full, C, None, pal)
    pair(lambda cm: cm.add_image(idx, labels, full, gt_palette=pal), lambda cm: cm.add_image(idx, labels, plane))
    pair(lambda cm: cm.add_view(r, cams[0], labels, to_device(full), gt_palette=pal), lambda cm: cm.add_view(r, cams[0], labels, plane))
    probs = rng.random((W, H, C), dtype=np.float32)
    pair(lambda cm: cm.add_probs(probs, full, gt_palette=pal), lambda cm: cm.add_probs(probs, plane))
    pair(lambda cm: cm.add_probs_many([probs], [to_device(full)], gt_palette=pal), lambda cm: cm.add_probs_many([probs], [plane]))
    with pytest.raises(ValueError, match="must have shape"):
        ConfusionMatrix(C).add_image(idx, labels, images[0], gt_palette=table)
