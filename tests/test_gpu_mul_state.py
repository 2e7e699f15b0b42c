"""The Mul aggregator's (hi, lo) accumulator ("Mul state", semantic_meshes_amd/csrc/fuse_tri.inc.hpp) over long runs, on every fold
path, against the numpy reference of tests/mul_state_ref.py (whose docstring derives the bound B; tests/test_mul_state_host.py
shows that B tells a dropped lo plane and float32 parts from the design, on these very inputs).

Observable: g = plane 0 + plane 1 of get_raw_rows, both read unfolded, in float64.  With k the reference's arg-max class of a row and
e the exact row, every finite element must satisfy

    |(g[c] - g[k]) - (e[c] - e[k])| <= 2 (B[c] + B[k])

(the factor 2: the device may sum a part in another order than the model, |t| then differs in its last bits; nothing else is allowed
for), non-finite elements must be the same -inf / +inf / NaN at the same places, and get() must agree at rtol 1e-5, atol 1e-6.
Re-centring: after every call the largest finite hi of a touched row is, in magnitude, at most the largest single-fold |part| the
reference saw for that row -- times (1 + 2^-24)^2 (1 + 2^-45): the centre class keeps its lo, at most 2^-24 of a hi that obeyed this
very limit, and the sum is rounded to float32 once.  That holds for every touched row with a finite member, rows with -inf, +inf or NaN
beside it included; the one exemption is the call in whose last fold of the row the class it was centred on itself left the finite
ones (the others then keep their distance to it until the row's next fold).  Every case asserts the path it is about.

Scenes of tests/mul_state_ref.py (CASES): at most 160 x 120 pixels, 48 x 36 for rows of 64 classes and more; 256 views for up to 48
classes, 64 for wider rows and for the run with non-finite members; eight ring cameras reused, every view its own class vectors, the views of
every other call a weights image.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mul_state_ref as R
from helpers import assert_fused_close

pytestmark = pytest.mark.gpu

SLACK = 2.0                                         # see above
RECENTRE = (1.0 + 2.0 ** -24) ** 2 * (1.0 + 2.0 ** -45)
SCATTER = os.environ.get("SMESH_ADD_RECORDS") == "0" or os.environ.get("SMESH_FUSE") == "strip"


def planes_of(agg):
    P = agg.primitives
    return agg.get_raw_rows(0, P, 0), agg.get_raw_rows(0, P, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_recentred(agg, ref, what):
    """After a call: the largest finite hi of every touched row that has a finite member (see the module's docstring)."""
    hi = agg.get_raw_rows(0, agg.primitives, 0).astype(np.float64)
    rows = (ref.views_touched > 0) & np.isfinite(ref.exact64()).any(axis=1) & ~ref.centre_lost
    assert np.isfinite(hi[rows]).any(axis=1).all(), what
    with np.errstate(invalid="ignore"):
        top = np.abs(np.where(np.isfinite(hi), hi, -np.inf).max(axis=1))
    bad = rows & ~(top <= ref.max_part * RECENTRE)
    assert not bad.any(), "%s: %d rows not re-centred, e.g. row %d: largest finite hi %.9g, largest |part| %.9g" % (
        what, int(bad.sum()), int(np.nonzero(bad)[0][0]), top[bad][0], ref.max_part[bad][0])


def assert_state(agg, ref, what, get=True):
    """The bound, the non-finite members and get(); returns the worst error / (B[c] + B[k])."""
    hi, lo = planes_of(agg)
    g = hi.astype(np.float64) + lo
    e = ref.exact64()
    assert R.same_class(g, e), "%s: non-finite members differ from the reference's" % what
    err, pb = ref.centred_error(g), ref.pair_bound()
    fin = np.isfinite(err)
    assert fin.sum() > fin.size // 4
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(fin & (err > 0), err / pb, 0.0)
    worst = float(ratio.max())
    print("%s: worst error / (B[c] + B[k]) = %.4g over %d finite elements, %d of them off the exact value" % (
        what, worst, int(fin.sum()), int((fin & (err > 0)).sum())))
    bad = fin & ~(err <= SLACK * pb)
    assert not bad.any(), "%s: %d elements beyond %g x the bound, worst ratio %.4g (row %d class %d: error %.4g, bound %.4g)" % (
        what, int(bad.sum()), SLACK, worst, *np.unravel_index(ratio.argmax(), ratio.shape), err.flat[ratio.argmax()], pb.flat[ratio.argmax()])
    if get:
        assert_fused_close(agg.get(), ref.get(), rtol=1e-5, atol=1e-6)
    return worst


def last_fuse(sm):
    return sm._lib.get_option("last_fuse_slot"), sm._lib.get_option("last_fuse_views")


def device_renderer(sm, cs):
    """The case's renderer; its index planes are the oracle's (the reference works on those)."""
    r = sm.render.texels(cs.mesh, cs.cams, R.TEXELS_PER_PIXEL) if cs.texels else sm.render.triangles(cs.mesh)
    assert r.getPrimitivesNum() == cs.P
    for cam, plane in zip(cs.cams, cs.planes):
        assert np.array_equal(np.asarray(r.render(cam, lazy=False)[0]).view(np.uint32), plane)
    return r


def run_calls(sm, cs, agg, ref, feed, first, last, what, after_call=None):
    """Views [first, last) in calls of cs.group views: the reference takes each view, `feed(cams, planes, probs, weights)` gives the
    call to the device (weights: a list, or None); the re-centring is checked after every call."""
    for start in range(first, last, cs.group):
        ids = list(range(start, min(start + cs.group, last)))
        inputs = [R.view_inputs(cs, i) for i in ids]
        for k, probs, weights in inputs:
            ref.add(cs.planes[k], probs, weights)
        weighted = [w is not None for _, _, w in inputs]
        assert all(weighted) or not any(weighted)
        feed([cs.cams[k] for k, _, _ in inputs], [cs.planes[k] for k, _, _ in inputs], [p for _, p, _ in inputs],
             [w for _, _, w in inputs] if weighted[0] else None)
        if after_call is not None:
            after_call()
        assert_recentred(agg, ref, "%s, views %d .. %d" % (what, ids[0], ids[-1]))


def fuse_views_feed(agg, r):
    from semantic_meshes_amd.device import to_device

    def feed(cams, planes, probs, weights):
        agg.fuse_views(r, cams, [to_device(p) for p in probs], None if weights is None else [to_device(w) for w in weights])
    return feed


def fuse_view_feed(agg, r):
    from semantic_meshes_amd.device import to_device

    def feed(cams, planes, probs, weights):
        for i, cam in enumerate(cams):
            agg.fuse_view(r, cam, to_device(probs[i]), None if weights is None else to_device(weights[i]))
    return feed


def add_feed(agg):
    def feed(cams, planes, probs, weights):
        for i, plane in enumerate(planes):
            agg.add(plane.copy(), probs[i], None if weights is None else weights[i])      # host copies: foreign index images
    return feed


def rasterised_case(sm, name, kernel, expect_queued, launch=None, per_view=False):
    from test_gpu_compact_records import queued
    from test_gpu_fuse_tri_instances import expected_launches
    cs = R.case(name)
    if not cs.texels:
        assert (queued(cs.mesh, cs.cams) > 0) == expect_queued
    r = device_renderer(sm, cs)
    agg = sm.fusion.MeshAggregator(cs.P, cs.C, "mul", cs.iew)
    agg.defer = False
    ref = R.MulReference(cs.P, cs.C, cs.iew, cs.fold_per)
    if launch is None:
        launch = expected_launches(cs.C, "mul", cs.group)[-1]

    def after_call():
        assert sm._lib.last_fuse_kernel() == kernel and sm._lib.last_add_path() == "render-records"
        if launch[0] is not None:
            assert last_fuse(sm) == launch, last_fuse(sm)
    run_calls(sm, cs, agg, ref, fuse_view_feed(agg, r) if per_view else fuse_views_feed(agg, r), 0, cs.views, name, after_call)
    assert (ref.views_touched * 2 >= cs.views).sum() >= 100
    return assert_state(agg, ref, name)


# ---- (a), (b), (g): k_fuse_tri -- small triangles, queued triangles (fuse_box), shuffled faces --------------------------------------
@pytest.mark.parametrize("name", ["a19", "a7", "a48"])
def test_small_triangles(sm, name):
    """(a) Every box within 8 x 8: the owner lane's fold in k_fuse_tri -- the exact instance of 19 classes, a run-time-C instance (7) and
    the 48-slot one, which takes two views per launch for Mul -- eight views per call, 256 views."""
    rasterised_case(sm, name, "k_fuse_tri", expect_queued=False)


def test_queued_triangles(sm):
    """(b) The closer ring: triangles over 8 x 8 are queued and fused by a wave each (fuse_box: per-lane double parts, wave_sum_d)."""
    rasterised_case(sm, "b19", "k_fuse_tri", expect_queued=True)


def test_shuffled_faces(sm):
    """(g) 4 320 faces handed over in shuffled order: the renderer re-orders them, rows are reached through its id table."""
    cs = R.case("g19")
    assert cs.P >= 4096
    rasterised_case(sm, "g19", "k_fuse_tri", expect_queued=True)


def test_one_two_four_and_eight_views_per_launch(sm):
    """(c) Fifteen views per call: launches of 8, 4, 2 and 1 views -- each translation unit's instance folds, eight calls."""
    from test_gpu_fuse_tri_instances import expected_launches
    from test_gpu_labels import fuse_slot_counts
    cs = R.case("c19")
    assert expected_launches(cs.C, "mul", cs.group) == [(19, 8), (19, 4), (19, 2), (19, 1)]
    r = device_renderer(sm, cs)
    agg = sm.fusion.MeshAggregator(cs.P, cs.C, "mul", cs.iew)
    ref = R.MulReference(cs.P, cs.C, cs.iew)
    feed = fuse_views_feed(agg, r)

    def counted(*args):
        assert fuse_slot_counts(sm, lambda: feed(*args)) == (4, 15)
        assert last_fuse(sm) == (19, 1) and sm._lib.last_fuse_kernel() == "k_fuse_tri"
    run_calls(sm, cs, agg, ref, counted, 0, cs.views, "c19")
    assert_state(agg, ref, "c19")


# ---- (d): any class count and wide rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel", [("d64", "k_fuse_tri_any"), ("d150", "k_fuse_tri_wide"), ("d520", "k_fuse_tri_wide")])
def test_any_class_count_and_wide_rows(sm, name, kernel):
    """(d) 64, 150 and 520 classes: the folds in slices of classes.  520 classes also send get() through k_mul_normalise.  (These
    launches re-centre the whole accumulator with k_mul_normalise ahead of their folds, as the generic scatter-add does: two splits of
    t per call, within the factor 2 of the assertion.)"""
    rasterised_case(sm, name, kernel, expect_queued=True, launch=(None, None))


# ---- (e): the texel renderer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_view", [("e5", False), ("e5big", True)])
def test_texel_renderer(sm, name, per_view):
    """(e) render.texels: small triangles through fuse_views (several views per launch), triangles of hundreds of pixels through
    fuse_view.  The texel kernels fold every pixel on its own (mul_fold_pixel): the bound counts a fold per contributing pixel.
    Which triangles go to k_fuse_texel_big is the rasteriser's box rule, worked out on the host: in e5 at most 7 of the 360 triangles
    have a box over 8 x 8 in any camera and hundreds stay within it, in e5big 20 and more of the 36 are over 8 x 8 in every camera."""
    from test_gpu_compact_records import kinds
    cs = R.case(name)
    ks = [kinds(cs.mesh, cam) for cam in cs.cams]
    big, small = [int((k == 2).sum()) for k in ks], [int(((k == 1) | (k == 3)).sum()) for k in ks]
    if per_view:
        assert min(big) >= 20 and len(cs.mesh.faces) == 36, big
    else:
        assert max(big) <= 7 and min(small) >= 100, (big, small)
    rasterised_case(sm, name, "k_fuse_texel", expect_queued=False, launch=(None, None), per_view=per_view)


# ---- (f): add() on foreign index images ----------------------------------------------------------------------------------------------
def test_foreign_index_images(sm):
    """(f) Host copies of the index planes: the records rebuilt from the image -- or, under SMESH_ADD_RECORDS=0 (the child process
    below), k_scatter_flat_mul's float64 atomics and k_fold_rows.  (That path re-centres the pair with k_mul_normalise ahead of its
    fold: the row's centre is then 0 when k_fold_rows looks for it, and a view splits t twice, 2 x 2^-48 |t| -- still within the
    factor 2 of the assertion, the 2^-53 terms of another summation order being four thousand times smaller.)"""
    cs = R.case("f19")
    agg = sm.fusion.MeshAggregator(cs.P, cs.C, "mul", cs.iew)
    ref = R.MulReference(cs.P, cs.C, cs.iew)

    def after_call():
        assert sm._lib.last_add_path() == ("scatter" if SCATTER else "image-records")
        assert sm._lib.last_fuse_kernel() == ("k_scatter_flat" if SCATTER else "k_fuse_tri")
    run_calls(sm, cs, agg, ref, add_feed(agg), 0, cs.views, "f19", after_call)
    assert_state(agg, ref, "f19 (%s)" % sm._lib.last_add_path())


def test_generic_scatter_in_a_child_process():
    """(f) SMESH_ADD_RECORDS=0 is read once per process: the case above again, through the generic scatter-add."""
    if SCATTER:
        pytest.skip("already on the scatter path")
    env = dict(os.environ, SMESH_ADD_RECORDS="0")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "test_foreign_index_images",
                          "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "1 passed" in res.stdout and "f19 (scatter)" in res.stdout, res.stdout[-1000:]
    print([line for line in res.stdout.splitlines() if line.startswith("f19")][-1])


def test_sparse_primitives_of_a_foreign_index_image(sm):
    """(f) Index images whose every primitive is scattered all over the image (tests/mul_state_ref.py, scattered_planes: the bounding
    box holds over ten times the 16 n + 256 pixels up to which image_records.hip scans a box): none of them is for the triangle-order
    kernels, their terms go through k_scatter_sparse's float64 atomics into the scratch rows and k_fold_sparse folds them, once per
    image, 256 images."""
    cs = R.case("sparse19")
    for plane in cs.planes:
        n, area = R.box_areas(plane, cs.P)
        assert (n > 8).all() and (area > 10 * (R.SPARSE_FACTOR * n + R.SPARSE_SLACK)).all()
    agg = sm.fusion.MeshAggregator(cs.P, cs.C, "mul", cs.iew)
    ref = R.MulReference(cs.P, cs.C, cs.iew)

    def after_call():
        assert sm._lib.last_add_path() == ("scatter" if SCATTER else "image-records")
    run_calls(sm, cs, agg, ref, add_feed(agg), 0, cs.views, "sparse19", after_call)
    assert (ref.views_touched == cs.views).all()
    assert_state(agg, ref, "sparse19")


# ---- a sequence of paths and readers on one aggregator ---------------------------------------------------------------------------
def test_sequence_of_paths_on_one_aggregator(sm):
    """fuse_views, add() of a foreign image, get() (the state untouched), fuse_view, get_raw() (the lo plane folded away), set_raw of
    the same values (nothing moves), 64 more views: the bound holds again, counted from the folded state."""
    from semantic_meshes_amd.device import to_device
    cs = R.case("s19")
    r = device_renderer(sm, cs)
    P, C = cs.P, cs.C
    agg = sm.fusion.MeshAggregator(P, C, "mul", cs.iew)
    agg.defer = False
    ref = R.MulReference(P, C, cs.iew)
    run_calls(sm, cs, agg, ref, fuse_views_feed(agg, r), 0, 16, "s19 fuse_views")
    assert sm._lib.last_fuse_kernel() == "k_fuse_tri" and last_fuse(sm) == (19, 8)
    k, probs, weights = R.view_inputs(cs, 16)
    ref.add(cs.planes[k], probs, weights)
    agg.add(cs.planes[k].copy(), probs, weights)
    assert sm._lib.last_add_path() == ("scatter" if SCATTER else "image-records")
    before = planes_of(agg)
    got = agg.get()
    after = planes_of(agg)
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
    assert before[1].any()
    assert_fused_close(got, ref.get(), rtol=1e-5, atol=1e-6)
    k, probs, weights = R.view_inputs(cs, 17)
    ref.add(cs.planes[k], probs, weights)
    agg.fuse_view(r, cs.cams[k], to_device(probs), None if weights is None else to_device(weights))
    assert last_fuse(sm) == (19, 1) and sm._lib.last_add_path() == "render-records"
    assert_recentred(agg, ref, "s19 fuse_view")
    assert_state(agg, ref, "s19 before get_raw")
    # get_raw(): the value rounded to the hi plane alone, the row centred on its largest element
    hi, lo = planes_of(agg)
    g = hi.astype(np.float64) + lo
    raw = agg.get_raw()
    hi2, lo2 = planes_of(agg)
    assert not lo2.any() and np.array_equal(bits(hi2), bits(raw))
    assert (raw.max(axis=1) == 0).all()
    kdev = g.argmax(axis=1)[:, None]
    e = ref.exact
    centred = (e - np.take_along_axis(e, kdev, 1)).astype(np.float64)
    ulp = np.spacing(np.abs(raw)).astype(np.float64)
    # what the pair itself was allowed before the fold (a device arg-max that is not the reference's: both pairs go through class k)
    kref = ref.argmax()[:, None]
    state = SLACK * (ref.bound + np.take_along_axis(ref.bound, kdev, 1) + np.where(kdev != kref, 2.0, 0.0) * np.take_along_axis(ref.bound, kref, 1))
    assert (np.abs(raw.astype(np.float64) - centred) <= ulp + state).all()
    assert (np.abs(raw.astype(np.float64) - centred) > 0).any()
    agg.set_raw(raw)
    again = agg.get_raw()
    hi3, lo3 = planes_of(agg)
    assert np.array_equal(bits(again), bits(raw)) and np.array_equal(bits(hi3), bits(raw)) and not lo3.any()
    # 64 more views from the folded state
    ref.rebase(raw)
    run_calls(sm, cs, agg, ref, fuse_views_feed(agg, r), 24, 88, "s19 after get_raw")
    assert_state(agg, ref, "s19 after get_raw")


# ---- non-finite members over a run -------------------------------------------------------------------------------------------------
def test_nonfinite_members_over_a_run(sm):
    """C = 5, iew = 0, 64 single-view calls (tests/mul_state_ref.py, nonfinite_edits): a class wiped by p = 0 in view 3 stays -inf and
    its row's finite classes keep the bound; a row that loses every class, at different views, is all -inf and get() gives zeros;
    p < 0 leaves NaN in its class only; p = +inf once; a zero weight over a p = 0 pixel adds nothing."""
    cs = R.case("n5")
    rows = R.nonfinite_rows()
    r = device_renderer(sm, cs)
    agg = sm.fusion.MeshAggregator(cs.P, cs.C, "mul", cs.iew)
    agg.defer = False
    ref = R.MulReference(cs.P, cs.C, cs.iew)

    def after_call():
        assert sm._lib.last_fuse_kernel() == "k_fuse_tri" and last_fuse(sm) == (5, 1)
        hi, lo = planes_of(agg)
        assert R.same_class(hi.astype(np.float64) + lo, ref.exact64()), "after view %d" % (ref.views - 1)
    run_calls(sm, cs, agg, ref, fuse_view_feed(agg, r), 0, cs.views, "n5", after_call)
    assert_state(agg, ref, "n5")
    hi, lo = planes_of(agg)
    g = hi.astype(np.float64) + lo
    assert np.isneginf(g[rows["wiped"]]).tolist() == [False, False, True, False, False]
    assert np.isneginf(g[rows["emptied"]]).all() and not agg.get()[rows["emptied"]].any()
    assert np.isnan(g[rows["negative"]]).tolist() == [False, True, False, False, False]
    assert np.isposinf(g[rows["infinite"]]).tolist() == [True, False, False, False, False]
    assert np.isfinite(g[rows["unweighted"]]).all()
    # the wiped row's finite classes were compared above: it has four of them
    assert np.isfinite(ref.centred_error(g)[rows["wiped"]]).sum() == 4


# ---- log_spec on the device ------------------------------------------------------------------------------------------------------
def sweep():
    """The values log_spec is fed (float32): every power of two, the mantissa boundaries at ten exponents, the ends of the denormal
    and normal ranges, 1 +- 1 ulp, FLT_MAX, 0, a negative value, +inf, and 4 096 random values of test_oracle's two distributions."""
    one = np.float32(1)
    powers = np.ldexp(np.float32(1), np.arange(-149, 128)).astype(np.float32)
    mant = np.array([(e << 23) | m for e in (1, 2, 31, 64, 100, 126, 127, 128, 200, 254) for m in (0, 0x3504F3, 0x3504F4, 0x7FFFFF)], np.uint32)
    special = np.concatenate([np.array([0x007FFFFF, 0x00800000, 0x7F7FFFFF], np.uint32).view(np.float32),
                              np.float32([np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), 0.0, -0.25, np.inf])])
    rng = np.random.default_rng(0)
    rand = np.concatenate([rng.random(2048, dtype=np.float32), np.exp(rng.uniform(-100, 88, 2048)).astype(np.float32)])
    x = np.concatenate([powers, mant.view(np.float32), special, rand]).astype(np.float32)
    assert len(powers) == 277 and powers[0] == np.float32(1e-45) and np.isfinite(powers).all() and (powers > 0).all()
    return x


def assert_same_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = ~nan & (bits(got) != bits(want))
    assert not bad.any(), "%s: %d values differ in bits, e.g. got %r want %r" % (what, int(bad.sum()), got[bad][0], want[bad][0])


@pytest.mark.parametrize("weighted", [False, True])
def test_log_spec_through_a_foreign_index_image(sm, weighted):
    """Mul, two classes, iew = 0, 64 x 64 pixels, idx = arange: class 0 holds the swept value, class 1 holds 1.  After one view from
    reset the hi plane is smesh_oracle_log_spec(x) in bits -- with a weights image float32(w * log_spec(x)), which a contracted
    multiply-add would change --, class 1 and the lo plane are 0."""
    W = H = 64
    P, C = W * H, 2
    x = sweep()
    x = np.concatenate([x, np.ones(-len(x) % P, np.float32)])
    rng = np.random.default_rng(1)
    agg = sm.fusion.MeshAggregator(P, C, "mul", 0.0)
    idx = np.arange(P, dtype=np.uint32).reshape(W, H)
    for lo in range(0, len(x), P):
        xs = x[lo:lo + P]
        probs = np.ones((W, H, C), np.float32)
        probs[:, :, 0] = xs.reshape(W, H)
        w = None
        if weighted:
            w = rng.random((W, H), dtype=np.float32)
            w[rng.random((W, H)) < 0.02] = 0.0
        agg.reset()
        agg.add(idx.copy(), probs, w)
        assert sm._lib.last_add_path() == ("scatter" if SCATTER else "image-records")
        hi, lo_plane = planes_of(agg)
        want = R.log_spec(xs) if w is None else R.mul_term(xs, w.reshape(-1))
        assert_same_bits(hi[:, 0], want, "values %d .." % lo)
        assert not hi[:, 1].any() and not lo_plane.any()


@pytest.mark.parametrize("C", [19, 7, 48])
def test_log_spec_through_the_rasteriser(sm, C):
    """1, 2, 4 and 8 views per launch (one translation unit each): the launch's last view carries class vectors, the views before it
    are all don't-care, so a row that owns exactly one pixel of the last view holds that pixel's terms,
    float32(w * log_spec(p)), in bits.  At least 100 such rows.  19 classes: the exact instance; 7: a run-time-C instance; 48: the
    48-slot instance, which exists for one and two views per launch only."""
    from semantic_meshes_amd.device import to_device
    cs = R.case("a19")
    r = device_renderer(sm, cs)
    P = cs.P
    W, H = cs.size
    rng = np.random.default_rng(2)
    agg = sm.fusion.MeshAggregator(P, C, "mul", cs.iew)
    zero = to_device(np.zeros((W, H, C), np.float32))
    for nv in ((1, 2) if C == 48 else (1, 2, 4, 8)):
        plane = cs.planes[nv - 1]
        n = np.bincount(plane[plane < P].astype(np.int64), minlength=P)
        xs, ys = np.nonzero((plane < P) & (n[np.minimum(plane, P - 1)] == 1))
        rows = plane[xs, ys]
        assert len(rows) >= 100
        probs = R.make_probs(rng, W, H, C)
        weights = [rng.random((W, H), dtype=np.float32) for _ in range(nv)]
        agg.reset()
        agg.fuse_views(r, cs.cams[:nv], [zero] * (nv - 1) + [to_device(probs)], [to_device(w) for w in weights])
        assert sm._lib.last_fuse_kernel() == "k_fuse_tri" and last_fuse(sm) == ({19: 19, 7: 8, 48: 48}[C], nv)
        hi, lo = planes_of(agg)
        p = probs[xs, ys]
        w = weights[-1][xs, ys]                                        # w0 = 0.5 * (1 / 1) + 0.5 = 1
        s = np.zeros(len(p), np.float32)
        for c in range(C):
            s = s + p[:, c]
        want = np.where((s > 0.5)[:, None], R.mul_term(p, w[:, None]), np.float32(0))
        assert (s > 0.5).sum() >= 90
        assert_same_bits(hi[rows].reshape(-1), want.reshape(-1), "%d views per launch" % nv)
        assert not lo[rows].any()
