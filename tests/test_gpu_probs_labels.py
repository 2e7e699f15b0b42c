"""The labels of a class-vector image and their confusion matrix on the device (include/smesh_probs_labels.h,
fusion.argmax_labels / argmax_labels_device, ConfusionMatrix.add_probs).

Every expectation is numpy: the explicit class loop of probs_labels_ref.ref_labels on the exactly widened image, and np.add.at for
the matrices.  Outputs are integers: all comparisons are array_equal.  Shapes are the smallest with runs shorter and longer than a
tile, W H not a multiple of one and a single-pixel tail; at these shapes every workgroup runs ONE round -- the largest, (130, 67) at 255
classes, is 363 tiles for a grid capped at a thousand or more.  The rounds after the first (the prefetch, the carry of the next
tile's pixel and ground truth, the grid-stride loop of the generic path) are tests/test_gpu_image_kernels_scale.py's."""
import ctypes

import numpy as np
import pytest

import probs_labels_ref as ref
from helpers import small_scene

pytestmark = pytest.mark.gpu

# (the issue's shapes, and (40, 9): with padded rows its runs of 9 pixels fill less than an eighth of a tile up to 83 classes (a tile
#  of 74 rows) and go to the generic path, from 84 classes on (72 rows) they are tiled; its runs of 40 are tiled throughout)
SHAPES = ((1, 1), (1, 7), (7, 1), (37, 53), (130, 67), (40, 9))
# Layouts the tiled path serves: the first three are ONE contiguous run; with padded rows every run has its own base (element-aligned
# only: the pad is 3 elements), its own head and tail, a last tile shorter than the others, and -- (7, 1), (1, 7), few classes -- runs
# under 32 bytes, which the generic path takes, beside longer ones.
TILEABLE = ("dense", "permuted", "offset", "padded rows", "padded rows permuted")
THRESHOLDS = (None, 0.9)


def class_counts():
    """The issue's list, and the last class count below and the first above every switch of the implementation: 23 / 24 (a tile holds
    256 rows / fewer), 63 / 64 (single pass with the small histogram / two passes), 83 / 84 (padded runs of 9 pixels: under an eighth
    of a tile, generic / tiled), the LDS limit of k_confusion, 255 / 256 (tiled / generic path)."""
    from semantic_meshes_amd import _lib, evaluation
    L, T = evaluation.lds_max_classes(), _lib.get_option("probs_labels_tile_max_classes")
    return sorted({1, 2, 3, 19, 20, 23, 24, 40, 63, 64, 83, 84, 150, L, L + 1, T, T + 1, 300})


N_COUNTS = 18


def test_the_class_count_list_is_the_one_the_parametrisation_assumes():
    assert len(class_counts()) == N_COUNTS and class_counts()[-1] == 300


@pytest.fixture(params=[1, 0], ids=["tiles", "generic"])
def tiles(request, sm):
    """Both paths: LDS tiles where the layout allows them / one lane per pixel everywhere."""
    before = sm._lib.get_option("probs_labels_tiles")
    sm._lib.set_option("probs_labels_tiles", request.param)
    yield request.param
    sm._lib.set_option("probs_labels_tiles", before)


@pytest.fixture(params=[0, 1], ids=["plain", "aggregate"])
def wave_aggregate(request, sm):
    before = sm._lib.get_option("confusion_wave_aggregate")
    sm._lib.set_option("confusion_wave_aggregate", request.param)
    yield request.param
    sm._lib.set_option("confusion_wave_aggregate", before)


_images = {}


def image(C, dtype, shape):
    """(values, widened, planted, {threshold: (labels, don't care)}) of one seeded image, made once and never changed."""
    key = (C, dtype, shape)
    if key not in _images:
        rng = np.random.default_rng([C, ref.DTYPES.index(dtype), shape[0], shape[1]])
        vals, wide, planted = ref.make_probs(rng, shape[0], shape[1], C, dtype)
        for a in (vals, wide):
            a.setflags(write=False)
        _images[key] = (vals, wide, planted, {t: ref.ref_labels(wide, t) for t in THRESHOLDS})
    return _images[key]


def kw(dtype):
    return {"probs_dtype": "bfloat16"} if dtype == "bfloat16" else {}


def expected_image(labels, dc, dc_value, out_dtype):
    return np.where(dc, dc_value, labels).astype(out_dtype)


def device_layout(vals, layout):
    """`vals` (W,H,C) on the device in one of the layouts of the issue, as the (W,H,C) view a user would pass."""
    from semantic_meshes_amd.device import DeviceArray, to_device
    W, H, C = vals.shape
    if layout == "dense":
        return to_device(vals)
    if layout == "permuted":            # a network's (H,W,C) tensor
        return to_device(np.ascontiguousarray(vals.transpose(1, 0, 2))).transpose(1, 0, 2)
    if layout == "offset":              # one element into a flat buffer: 4-byte / 2-byte alignment only
        flat = np.zeros(vals.size + 1, vals.dtype)
        flat[1:] = vals.ravel()
        buf = to_device(flat)
        return DeviceArray(buf.ptr + vals.dtype.itemsize, (W, H, C), vals.dtype, buf.device, owner=buf)
    if layout == "padded rows":         # (W,H,C) rows of H C elements, 3 elements apart: runs along y
        rows = np.zeros((W, H * C + 3), vals.dtype)
        rows[:, :H * C] = vals.reshape(W, H * C)
        buf = to_device(rows)
        return DeviceArray(buf.ptr, (W, H, C), vals.dtype, buf.device, (H * C + 3, C, 1), owner=buf)
    if layout == "padded rows permuted":   # a (H,W,C) tensor with padded rows seen as (W,H,C): runs along x
        rows = np.zeros((H, W * C + 3), vals.dtype)
        rows[:, :W * C] = vals.transpose(1, 0, 2).reshape(H, W * C)
        buf = to_device(rows)
        return DeviceArray(buf.ptr, (W, H, C), vals.dtype, buf.device, (C, W * C + 3, 1), owner=buf)
    if layout == "class stride 2":
        wide = np.zeros((W, H, 2 * C), vals.dtype)
        wide[..., ::2] = vals
        buf = to_device(wide)
        return DeviceArray(buf.ptr, (W, H, C), vals.dtype, buf.device, (H * 2 * C, 2 * C, 2), owner=buf)
    if layout == "channel first":       # (C,H,W) seen as (W,H,C)
        return to_device(np.ascontiguousarray(vals.transpose(2, 1, 0))).transpose(2, 1, 0)
    raise KeyError(layout)


def check_labels(sm, C, dtype, shape, layout, thr):
    vals, wide, planted, want = image(C, dtype, shape)
    lab, dc = want[thr]
    out_dt = np.uint8 if C <= 255 else np.uint16
    dev = device_layout(vals, layout)
    got = sm.fusion.argmax_labels_device(dev, dont_care_threshold=thr, **kw(dtype))
    assert got.shape == shape and got.dtype == out_dt
    if layout in ("permuted", "channel first", "padded rows permuted") and min(shape) > 1:
        assert got.strides == (1, shape[0])                # the output follows the input's pixel order
    elif layout == "dense":
        assert got.strides == (shape[1], 1)
    assert np.array_equal(got.numpy(), expected_image(lab, dc, np.iinfo(out_dt).max, out_dt)), (C, dtype, shape, layout, thr)
    return dev


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("which", range(N_COUNTS))
def test_tileable_layouts_on_both_paths(sm, which, dtype, tiles):
    C = class_counts()[which]
    for shape in SHAPES:
        vals, wide, planted, want = image(C, dtype, shape)
        if shape[0] * shape[1] >= 12 and C >= 3:           # every planted case is there, and the threshold has both sides
            assert len(planted) == 12
            for name, x, y in planted:
                assert ref.is_planted(name, wide[x, y]), (name, dtype)
            nan_sum = [(x, y) for name, x, y in planted if name.startswith("NaN")]
            assert nan_sum and not any(want[0.9][1][x, y] for x, y in nan_sum)          # a NaN sum comes out labelled
            assert 0.15 < want[0.9][1].mean() < 0.6 and not want[None][1].any()
            assert len(np.unique(want[None][0])) > 1
        for layout in TILEABLE:
            for thr in THRESHOLDS:
                check_labels(sm, C, dtype, shape, layout, thr)


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("which", range(N_COUNTS))
def test_layouts_of_the_generic_path(sm, which, dtype):
    from semantic_meshes_amd.device import DeviceArray, to_device
    C = class_counts()[which]
    for shape in SHAPES:
        for layout in ("class stride 2", "channel first"):
            for thr in THRESHOLDS:
                check_labels(sm, C, dtype, shape, layout, thr)
        # a zero class stride: every class of a pixel is the same element -- label 0, and the sum is C additions of it
        vals, wide, _, _ = image(C, dtype, shape)
        W, H = shape
        plane = to_device(np.ascontiguousarray(vals[..., 0]))
        view = DeviceArray(plane.ptr, (W, H, C), vals.dtype, plane.device, (H, 1, 0), owner=plane)
        for thr in THRESHOLDS:
            lab, dc = ref.ref_labels(np.broadcast_to(wide[..., :1], (W, H, C)), thr)
            assert not lab.any()
            got = sm.fusion.argmax_labels(view, dont_care_threshold=thr, **kw(dtype))
            assert np.array_equal(got, np.where(dc, 255 if C <= 255 else 65535, 0)), (C, dtype, shape, thr)


def test_host_images_output_dtypes_and_dont_care_labels(sm, tiles):
    for C, dtype, shape in ((19, "float32", (37, 53)), (40, "float16", (130, 67)), (300, "bfloat16", (37, 53)), (3, "float16", (1, 7))):
        vals, wide, _, want = image(C, dtype, shape)
        lab, dc = want[0.9]
        hosts = [vals, np.ascontiguousarray(vals.transpose(1, 0, 2)).transpose(1, 0, 2), np.ascontiguousarray(vals.transpose(2, 1, 0)).transpose(2, 1, 0)]
        for h in hosts:                                    # a host image crosses at its own width, whatever its strides
            got = sm.fusion.argmax_labels(h, dont_care_threshold=0.9, **kw(dtype))
            assert got.dtype == (np.uint8 if C <= 255 else np.uint16)
            assert np.array_equal(got, expected_image(lab, dc, np.iinfo(got.dtype).max, got.dtype))
        if dtype == "float32":                             # a float64 host image is converted, as add() does
            got = sm.fusion.argmax_labels(vals.astype(np.float64), dont_care_threshold=0.9)
            assert np.array_equal(got, expected_image(lab, dc, 255, np.uint8))
        for out_dt, dcv in ((np.int32, -1), (np.int32, C), (np.uint16, 65535), (np.uint16, C + 1)) + (((np.uint8, 254),) if C < 254 else ()):
            got = sm.fusion.argmax_labels(vals, dont_care_threshold=0.9, dont_care_label=dcv, dtype=out_dt, **kw(dtype))
            assert got.dtype == out_dt and np.array_equal(got, expected_image(lab, dc, dcv, out_dt)), (C, out_dt, dcv)


# ---- add_probs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(N_COUNTS))
def test_add_probs(sm, which, wave_aggregate, tiles):
    from semantic_meshes_amd.device import to_device
    C = class_counts()[which]
    rng = np.random.default_rng(500 + which)
    cm = sm.fusion.ConfusionMatrix(C)
    k = which
    for shape in SHAPES:
        for dtype in ref.DTYPES:
            vals, wide, _, want = image(C, dtype, shape)
            thr = THRESHOLDS[k % 2]
            gdt = ref.LBL_DTYPES[k % len(ref.LBL_DTYPES)]
            k += 1
            lab, dc = want[thr]
            gt = ref.make_gt(rng, shape, C, gdt)
            M, ignored = ref.expected_matrix(np.where(dc, -1, lab), gt, C)
            if shape[0] * shape[1] > 1000 and C > 1:
                assert (thr is None or M[:, C].sum() > 0) and (np.iinfo(gt.dtype).max < C + 7 or ignored > 0)
            gt_hw = np.ascontiguousarray(gt.T)
            for probs, g in ((device_layout(vals, "dense"), gt),                              # host ground truth
                             (device_layout(vals, "permuted"), to_device(gt_hw).T),           # (H,W) images on the device
                             (device_layout(vals, "offset"), to_device(gt)),
                             (device_layout(vals, "padded rows"), to_device(gt)),             # one run per row ...
                             (device_layout(vals, "padded rows permuted"), to_device(gt_hw).T),  # ... along either axis
                             (vals, gt_hw.T),                                                  # everything on the host
                             (device_layout(vals, "channel first"), to_device(gt))):          # the generic path
                cm.reset()
                cm.add_probs(probs, g, dont_care_threshold=thr, **kw(dtype))
                assert np.array_equal(cm.get(), M) and cm.ignored == ignored, (C, shape, dtype, gdt, thr)


@pytest.mark.parametrize("C", [19, 64, 300])
def test_add_probs_accumulates_with_the_other_calls_and_returns_its_labels(sm, C, tiles):
    from semantic_meshes_amd.device import to_device
    rng = np.random.default_rng(600 + C)
    shape = (130, 67)
    cm = sm.fusion.ConfusionMatrix(C)
    total, total_ignored = np.zeros((C, C + 1), np.uint64), 0
    outs = []
    for dtype in ref.DTYPES:
        vals, wide, _, want = image(C, dtype, shape)
        lab, dc = want[0.9]
        gt = ref.make_gt(rng, shape, C, "int16")
        M, ign = ref.expected_matrix(np.where(dc, -1, lab), gt, C)
        total, total_ignored = total + M, total_ignored + ign
        dev = device_layout(vals, "permuted" if dtype == "float16" else "dense")
        out = cm.add_probs(dev, to_device(gt), dont_care_threshold=0.9, labels_out=True, **kw(dtype))
        assert out.shape == shape and out.strides == ((1, shape[0]) if dtype == "float16" else (shape[1], 1))
        outs.append((out, dev, dtype))
    # ... then an index image and a 1-D call on the same matrix
    P = 50
    idx = rng.integers(0, P + 5, size=shape).astype(np.uint32)
    table = rng.integers(-1, C, size=P).astype(np.int32)
    gt = ref.make_gt(rng, shape, C, "uint8")
    pred = np.where(idx < P, table[np.minimum(idx, P - 1)], -1)
    M, ign = ref.expected_matrix(pred, gt, C)
    cm.add_image(idx, table, gt)
    total, total_ignored = total + M, total_ignored + ign
    p1, g1 = rng.integers(-1, C + 1, size=3001).astype(np.int32), ref.make_gt(rng, 3001, C, "int32")
    M, ign = ref.expected_matrix(p1, g1, C)
    cm.add(p1, g1)
    total, total_ignored = total + M, total_ignored + ign
    assert np.array_equal(cm.get(), total) and cm.ignored == total_ignored
    for out, dev, dtype in outs:                           # the label image of the same pass is argmax_labels'
        want = sm.fusion.argmax_labels(dev, dont_care_threshold=0.9, **kw(dtype))
        assert out.dtype == want.dtype and np.array_equal(out.numpy(), want)
    lists = cm.add_probs_many([d for _, d, _ in outs[:1]], [to_device(gt)], labels_out=True)
    assert len(lists) == 1 and np.array_equal(lists[0].numpy(), sm.fusion.argmax_labels(outs[0][1]))


# ---- composition: hard-vote fusion of soft predictions -------------------------------------------------------------------------------
def test_add_labels_of_the_argmax_equals_add_of_its_one_hot(sm):
    from semantic_meshes_amd.device import to_device
    C = 19
    # (finely tessellated: every bounding box at most 8 x 8 pixels, so one lane owns each row and the float32 sums have one order --
    #  the triangles a coarser scene queues are summed by float atomics in no fixed order, in both calls)
    mesh, cams = small_scene(a=160, b=80)
    P = len(mesh.faces)
    r = sm.render.triangles(mesh)
    for cam in cams:
        r.render(cam)
        assert r.render_stats(cam, queues=True)[1][0] == 0
    a, b = sm.fusion.MeshAggregator(P, C), sm.fusion.MeshAggregator(P, C)
    for k, cam in enumerate(cams):
        dtype = ref.DTYPES[k % 3]
        rng = np.random.default_rng(700 + k)
        vals, wide, _ = ref.make_probs(rng, cam.resolution[0], cam.resolution[1], C, dtype)
        lab, dc = ref.ref_labels(wide, 0.9)
        a.add_labels(r.render(cam)[0], sm.fusion.argmax_labels_device(to_device(vals), dont_care_threshold=0.9, **kw(dtype)))
        b.add(r.render(cam)[0], to_device(ref.one_hot(np.where(dc, -1, lab), C)))
    ga, gb = a.get(), b.get()
    assert np.nan_to_num(gb).any() and np.array_equal(ga, gb, equal_nan=True)


# ---- every SMESH_ERR_INVALID of the header ------------------------------------------------------------------------------------------
def test_invalid_calls_are_refused_and_change_nothing(sm):
    from semantic_meshes_amd.device import to_device
    L = sm._lib
    lib = L.lib()
    C, (W, H) = 19, (37, 53)
    vals, wide, _, want = image(C, "float32", (W, H))
    rng = np.random.default_rng(800)
    gt = ref.make_gt(rng, (W, H), C, "uint8")
    d_probs, d_gt = to_device(vals), to_device(gt)
    sentinel = np.full((W, H), 77, np.int32)
    d_out = to_device(sentinel)
    cm = sm.fusion.ConfusionMatrix(C)
    cm.add_probs(d_probs, d_gt)
    before, ignored = cm.get(), cm.ignored
    assert before.any()
    c64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    vp = ctypes.c_void_p
    U8, U16, I32, I8, F32, DEV, HOST, ninf = L.LBL_CODES["uint8"], L.LBL_CODES["uint16"], L.LBL_CODES["int32"], L.LBL_CODES["int8"], L.PROBS_F32, L.MEM_DEVICE, L.MEM_HOST, float("-inf")

    def labels(probs=d_probs.ptr, pdt=F32, pstr=None, pmem=DEV, w=W, h=H, c=C, thr=ninf, out=d_out.ptr, odt=I32, ostr=None, dcv=-1, omem=DEV, device=0):
        return lib.smesh_probs_labels(vp(probs), pdt, pstr, pmem, w, h, c, thr, vp(out), odt, ostr, dcv, omem, device)

    def add(h_=None, probs=d_probs.ptr, pdt=F32, pstr=None, pmem=DEV, g=d_gt.ptr, gdt=U8, gstr=None, gmem=DEV, w=W, h=H, thr=ninf,
            out=None, odt=I32, ostr=None, dcv=-1):
        return lib.smesh_confusion_add_probs(cm._h if h_ is None else h_, vp(probs), pdt, pstr, pmem, vp(g), gdt, gstr, gmem, w, h, thr,
                                             None if out is None else vp(out), odt, ostr, dcv)

    assert labels() == L.OK and add(out=d_out.ptr) == L.OK         # the well-formed calls these are variations of
    assert np.array_equal(d_out.numpy(), want[None][0])
    cm.reset()
    cm.add_probs(d_probs, d_gt)
    d_out = to_device(sentinel)
    bad = [
        lambda: labels(probs=0), lambda: labels(out=0),
        lambda: labels(pdt=3), lambda: labels(pdt=-1),
        lambda: labels(pstr=c64(-1, C, 1)), lambda: labels(pstr=c64(H * C, C, -1)),
        lambda: labels(pmem=2), lambda: labels(omem=7),
        lambda: labels(c=0),
        lambda: labels(thr=float("nan")),
        lambda: labels(w=65537, h=1), lambda: labels(w=1 << 15, h=1 << 14),             # W H = 2^29
        lambda: labels(probs=d_probs.ptr + 2),                                          # not aligned to a float32
        lambda: labels(odt=I8), lambda: labels(odt=L.LBL_CODES["int64"]), lambda: labels(odt=99),
        lambda: labels(ostr=c64(-H, 1)),
        lambda: labels(odt=U8, dcv=255, c=256),                                         # too narrow for C
        lambda: labels(odt=U16, dcv=65535, c=65536),
        lambda: labels(dcv=0), lambda: labels(dcv=C - 1),                               # a class
        lambda: labels(odt=U8, dcv=256), lambda: labels(odt=U8, dcv=-1), lambda: labels(odt=U16, dcv=65536), lambda: labels(dcv=1 << 31),
        lambda: labels(device=4096),
        lambda: add(h_=vp(0)),
        lambda: add(probs=0), lambda: add(g=0),
        lambda: add(pdt=5), lambda: add(gdt=8), lambda: add(gdt=-1),
        lambda: add(pstr=c64(H * C, -C, 1)), lambda: add(gstr=c64(-1, 1)),
        lambda: add(pmem=3), lambda: add(gmem=-1),
        lambda: add(thr=float("nan")),
        lambda: add(w=65537, h=1),
        lambda: add(out=d_out.ptr, odt=U8, dcv=3), lambda: add(out=d_out.ptr, odt=I8), lambda: add(out=d_out.ptr, ostr=c64(1, -1)),
        lambda: add(out=d_out.ptr, odt=U8, dcv=300),
    ]
    for k, call in enumerate(bad):
        assert call() == L.ERR_INVALID, k
        assert lib.smesh_last_error(), k
    assert np.array_equal(cm.get(), before) and cm.ignored == ignored
    assert np.array_equal(d_out.numpy(), sentinel)
    # an empty image is nothing to do; the arguments of an absent label image are not looked at
    assert labels(w=0) == L.OK and add(h=0) == L.OK and add(odt=99, dcv=0) == L.OK
    assert np.array_equal(cm.get(), before * np.uint64(2))


def test_profile_slot_brackets_the_kernel(sm):
    from semantic_meshes_amd.device import to_device
    L = sm._lib
    lib = L.lib()
    vals, _, _, _ = image(19, "float32", (130, 67))
    dev, gt = to_device(vals), to_device(np.zeros((130, 67), np.uint8))
    L.check(lib.smesh_profile_reset(0))
    L.check(lib.smesh_profile_sample_every(0, 1))
    L.check(lib.smesh_profile_enable(0, 1 << L.PROF_PROBS_LABELS))
    try:
        sm.fusion.argmax_labels_device(dev)
        cm = sm.fusion.ConfusionMatrix(19)
        cm.add_probs(dev, gt)
        cm.get()
        L.synchronize(0)
        ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
        L.check(lib.smesh_profile_read(0, L.PROF_PROBS_LABELS, ctypes.byref(ms), ctypes.byref(n)))
        assert n.value == 2 and ms.value > 0
    finally:
        L.check(lib.smesh_profile_enable(0, 0))
