"""Reference of the Mul aggregator's (hi, lo) state ("Mul state", semantic_meshes_amd/csrc/fuse_tri.inc.hpp), in numpy, for
tests/test_mul_state_host.py (no GPU) and tests/test_gpu_mul_state.py.

Terms.  A pixel's float32 term of class c is w * log_spec(p[c]); log_spec is the oracle's copy of the spec's logarithm
(smesh_oracle_log_spec, pinned against np.log in tests/test_oracle.py); w0 = iew * (1.0f / n) + (1 - iew) and w = w0 * wt, every
operation rounded to float32; n is the number of the primitive's pixels in the index plane, don't-care pixels included.  A pixel
contributes when the sequential float32 sum of its classes is > 0.5; w == 0 contributes nothing.

Exact state.  Per view and row, `part` is the sum of the view's terms in float64 (the terms are float32 numbers: the sum of a few
hundred of them in double is exact to n * 2^-53); across views the parts accumulate in np.longdouble.

Model of the device state (for the bound alone), in float64: centre m = the largest finite hi of the row before the fold,
t = ((hi - m) + lo) + part, hi = float32(t), lo = float32(t - hi) where hi is finite, else 0.

Bound.  B[r, c] = sum over the folds of 2^-48 |t| + n 2^-53 |part|: the first summand is the one rounding mul_fold makes when it
splits t into two float32 (|t - hi| <= 2^-24 |t|, and its float32 rounding loses at most 2^-24 of that), the second a double
summation of n terms in any order.  `fold="pixel"` folds every contributing pixel on its own, in image order: what the texel kernels
of one and of several views do (mul_fold_pixel), and an upper bound of the big texel triangles' one fold per view.

Broken models (for the host test: what the bound must tell apart).  B: the lo plane dropped, a float32 hi alone.  C: a view's part
summed sequentially in float32, then folded as the model does.
"""
import ctypes
import functools
import types

import numpy as np

from helpers import random_probs

F32 = np.float32
EPS48, EPS53 = 2.0 ** -48, 2.0 ** -53


def log_spec(x):
    """smesh_oracle_log_spec, vectorised: float32 in, float32 out, any shape."""
    from oracle import oracle
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    oracle.lib().smesh_oracle_log_spec(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(x.size))
    return out


def mul_term(p, w):
    """float32(w * log_spec(p)), 0 where w == 0 (log_of_power)."""
    p, w = np.asarray(p, np.float32), np.asarray(w, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (w * log_spec(p)).astype(np.float32)
    return np.where(w == 0, F32(0), t)


def view_terms(idx, probs, weights, P, iew):
    """One view: (n, rows, terms, rank) -- n[P] pixels per primitive in the index plane; for the contributing pixels, in image order
    within a row and sorted by row: their rows, their float32 terms [m, C] and their position among the row's contributing pixels."""
    C = probs.shape[-1]
    flat = np.asarray(idx).reshape(-1).astype(np.int64)
    inside = (flat >= 0) & (flat < P)
    n = np.bincount(flat[inside], minlength=P)
    pr = np.asarray(probs, np.float32).reshape(-1, C)
    s = np.zeros(len(pr), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            s = s + pr[:, c]                                           # sequential float32, class order
    iew = F32(iew)
    w0 = (iew * (F32(1) / np.maximum(n, 1).astype(np.float32)) + (F32(1) - iew) * F32(1)).astype(np.float32)
    safe = np.where(inside, flat, 0)
    w = w0[safe] if weights is None else (w0[safe] * np.asarray(weights, np.float32).reshape(-1)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        take = np.nonzero(inside & (s > F32(0.5)) & (w != 0))[0]
    take = take[np.argsort(flat[take], kind="stable")]
    rows = flat[take]
    terms = mul_term(pr[take], w[take][:, None])
    start = np.nonzero(np.r_[True, rows[1:] != rows[:-1]])[0] if len(rows) else np.zeros(0, np.int64)
    rank = np.arange(len(rows)) - np.repeat(start, np.diff(np.r_[start, len(rows)])) if len(rows) else np.zeros(0, np.int64)
    return n, rows, terms, rank


def sum_by_row(rows, values, P):
    """values [m, C] summed per row (rows sorted) into [P, C], in values' dtype: float64 -- any order --, float32 -- sequential."""
    out = np.zeros((P, values.shape[1]), values.dtype)
    if not len(rows):
        return out
    start = np.nonzero(np.r_[True, rows[1:] != rows[:-1]])[0]
    with np.errstate(invalid="ignore", over="ignore"):
        if values.dtype == np.float64:
            out[rows[start]] = np.add.reduceat(values, start, axis=0)
        else:
            rank = np.arange(len(rows)) - np.repeat(start, np.diff(np.r_[start, len(rows)]))
            for k in range(int(rank.max()) + 1):
                sel = rank == k
                out[rows[sel]] = out[rows[sel]] + values[sel]
    return out


def centre_of(hi):
    """Largest finite element per row, 0 where there is none (row_centre)."""
    m = np.where(np.isfinite(hi), hi, -np.inf).max(axis=1)
    return np.where(m > -np.inf, m, 0.0)


def fold(hi, lo, part):
    """mul_fold on whole rows in float64: (hi, lo, t) after the fold, the row shifted by its centre."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((hi - centre_of(hi)[:, None]) + lo) + part
        h = t.astype(np.float32).astype(np.float64)
        fin = np.isfinite(h)
        l = np.where(fin, (t - np.where(fin, h, 0.0)).astype(np.float32).astype(np.float64), 0.0)
    return h, l, t


class MulReference:
    """The exact rows, the model of the device state with its bound, and -- with `broken` -- the two broken models."""

    def __init__(self, P, C, iew, fold_per="view", broken=False):
        self.P, self.C, self.iew, self.fold_per, self.broken = int(P), int(C), float(iew), fold_per, broken
        self.reset()

    def reset(self):
        P, C = self.P, self.C
        self.exact = np.zeros((P, C), np.longdouble)
        self.hi, self.lo, self.bound = np.zeros((P, C)), np.zeros((P, C)), np.zeros((P, C))
        self.max_part = np.zeros(P)          # largest finite |part| of a single fold so far, per row
        self.centre_lost = np.zeros(P, bool)  # see _fold
        self.views_touched = np.zeros(P, np.int64)
        self.first_fold = np.full(P, -1, np.int64)   # the view of a row's first fold
        self.views = 0
        if self.broken:
            self.hi_b = np.zeros((P, C))
            self.hi_c, self.lo_c = np.zeros((P, C)), np.zeros((P, C))

    def rebase(self, hi):
        """The device state was folded to the hi plane alone (get_raw): the exact rows and the bound are counted from `hi` on."""
        self.exact = np.asarray(hi, np.float64).astype(np.longdouble)
        self.hi, self.lo, self.bound = np.asarray(hi, np.float64).copy(), np.zeros((self.P, self.C)), np.zeros((self.P, self.C))

    def _fold(self, rows, part, nterms, part32=None):
        before = self.hi[rows]
        leader = np.where(np.isfinite(before), before, -np.inf).argmax(axis=1)[:, None]
        h, l, t = fold(before, self.lo[rows], part)
        self.hi[rows], self.lo[rows] = h, l
        # the class the row was centred on left the finite ones in this very fold: the rest keep their distance to it, whatever its
        # size, until the row's next fold centres them on their own largest
        self.centre_lost[rows] = ~np.isfinite(np.take_along_axis(h, leader, 1))[:, 0]
        with np.errstate(invalid="ignore"):
            b = EPS48 * np.abs(t) + nterms[:, None] * EPS53 * np.abs(part)
            self.bound[rows] += np.where(np.isfinite(b), b, 0.0)
            self.exact[rows] += part.astype(np.longdouble)
            mp = np.where(np.isfinite(part), np.abs(part), 0.0).max(axis=1)
        self.max_part[rows] = np.maximum(self.max_part[rows], mp)
        if self.broken:
            hb = self.hi_b[rows]
            with np.errstate(invalid="ignore", over="ignore"):
                self.hi_b[rows] = ((hb - centre_of(hb)[:, None]) + part).astype(np.float32).astype(np.float64)
            self.hi_c[rows], self.lo_c[rows], _ = fold(self.hi_c[rows], self.lo_c[rows], part32.astype(np.float64))

    def add(self, idx, probs, weights=None):
        n, rows, terms, rank = view_terms(idx, probs, weights, self.P, self.iew)
        touched = np.nonzero(n > 0)[0]
        fresh = touched[self.first_fold[touched] < 0]
        self.first_fold[fresh] = self.views
        self.views_touched[touched] += 1
        self.views += 1
        self.last_n = n
        if self.fold_per == "view":
            part = sum_by_row(rows, terms.astype(np.float64), self.P)[touched]
            part32 = sum_by_row(rows, terms, self.P)[touched] if self.broken else None
            self._fold(touched, part, n[touched].astype(np.float64), part32)
        else:
            # (the texel kernel of big triangles folds a view's sum at once: `max_part` covers that too)
            whole = sum_by_row(rows, terms.astype(np.float64), self.P)[touched]
            with np.errstate(invalid="ignore"):
                self.max_part[touched] = np.maximum(self.max_part[touched], np.where(np.isfinite(whole), np.abs(whole), 0.0).max(axis=1))
            for k in range(int(rank.max()) + 1 if len(rank) else 0):
                sel = rank == k
                self._fold(rows[sel], terms[sel].astype(np.float64), np.ones(int(sel.sum())), terms[sel])

    # ---- what the tests compare ----------------------------------------------------------------------------------------------------
    def exact64(self):
        return self.exact.astype(np.float64)

    def argmax(self):
        """The arg-max class of every exact row (the lowest among equals; NaN never wins, -inf only in a row of nothing else)."""
        e = self.exact64()
        return np.where(np.isnan(e), -np.inf, e).argmax(axis=1)

    def centred_error(self, values):
        """|(v[c] - v[k]) - (e[c] - e[k])| per element, k the reference's arg-max class; NaN where either side is not finite."""
        k = self.argmax()[:, None]
        e = self.exact
        v = np.asarray(values).astype(np.longdouble)
        with np.errstate(invalid="ignore"):
            d = np.abs((v - np.take_along_axis(v, k, 1)) - (e - np.take_along_axis(e, k, 1))).astype(np.float64)
        return d

    def pair_bound(self):
        """B[c] + B[k]."""
        k = self.argmax()[:, None]
        return self.bound + np.take_along_axis(self.bound, k, 1)

    def get(self):
        """get() of the exact rows in float64: exp(row - max) L1-normalised, NaN / Inf -> 0 (the oracle's get_rows)."""
        e = self.exact64()
        m = e[:, 0].copy()
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for c in range(1, self.C):
                m = np.where(e[:, c] > m, e[:, c], m)
            x = np.exp(e - m[:, None])
            out = x / np.abs(x).sum(axis=1, keepdims=True)
        return np.where(np.isfinite(out), out, 0.0)


def same_class(values, exact):
    """Non-finite elements: -inf, +inf and NaN at the same places on both sides."""
    v, e = np.asarray(values, np.float64), np.asarray(exact, np.float64)
    return (np.array_equal(np.isnan(v), np.isnan(e)) and np.array_equal(np.isposinf(v), np.isposinf(e))
            and np.array_equal(np.isneginf(v), np.isneginf(e)))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def make_probs(rng, W, H, C, zero_fraction=0.05, near_one=0.05):
    """helpers.random_probs, and in about `near_one` of the pixels that are not don't-care one class within 2^-12 of 1: its term is
    about -2^-13 with 24 significant bits beside sums of magnitude 10 .. 1000, so t needs more than 48 bits and the fold rounds."""
    p = random_probs(rng, W, H, C, zero_fraction)
    sel = (rng.random((W, H)) < near_one) & (p.sum(axis=-1) > 0.5)
    cls = rng.integers(0, C, (W, H))
    val = (F32(1) - rng.random((W, H), dtype=np.float32) * F32(2.0 ** -12)).astype(np.float32)
    xs, ys = np.nonzero(sel)
    p[xs, ys, cls[xs, ys]] = val[xs, ys]
    return p


def view_inputs(case, i):
    """View i of a run: (camera slot, class vectors, weights image or None) -- every view its own class vectors; the views of every
    other call (of `case.group` views: a call's views have weights images or none has) a weights image."""
    rng = np.random.default_rng([case.seed, i])
    W, H = case.size
    probs = make_probs(rng, W, H, case.C)
    weights = (rng.random((W, H), dtype=np.float32) + F32(0.25)).astype(np.float32) if (i // case.group) % 2 else None
    if case.name == "n5":
        nonfinite_edits(case, i, probs, weights)
    return i % len(case.cams), probs, weights


# name: (mesh, ring scale, (W, H), C, views, fold_per, iew, views per call).  Meshes: fine_grid arguments; "shuffled": the grid with
# permuted faces; "texels": a texel renderer on the grid.  Scenes: in every row that at least half of the views touch, some camera
# sees more than one pixel (a row of single pixels cannot tell a float32 sum of a view's terms from a float64 one).
CASES = {
    "a19": (("grid", 70, 15), 0.62, (160, 120), 19, 256, "view", 0.5, 8),
    "a7": (("grid", 70, 15), 0.62, (160, 120), 7, 256, "view", 0.5, 8),
    "a48": (("grid", 70, 15), 0.62, (160, 120), 48, 256, "view", 0.5, 8),
    "b19": (("grid", 100, 15), "wide", (160, 120), 19, 256, "view", 0.5, 8),
    "c19": (("grid", 70, 15), 0.62, (160, 120), 19, 120, "view", 0.5, 15),
    "d64": (("grid", 30, 6), "wide", (48, 36), 64, 64, "view", 0.5, 8),
    "d150": (("grid", 30, 6), "wide", (48, 36), 150, 64, "view", 0.5, 8),
    "d520": (("grid", 30, 6), "wide", (48, 36), 520, 64, "view", 0.5, 8),
    "e5": (("texels", 30, 6), 0.62, (96, 72), 5, 256, "pixel", 0.5, 8),
    "e5big": (("texels", 6, 3), "wide", (96, 72), 5, 256, "pixel", 0.5, 1),
    "f19": (("grid", 70, 15), 0.62, (160, 120), 19, 256, "view", 0.5, 1),
    "g19": (("shuffled", 90, 24), "wide", (160, 120), 19, 256, "view", 0.5, 8),
    "s19": (("grid", 70, 15), 0.62, (160, 120), 19, 16 + 1 + 1 + 64, "view", 0.5, 8),
    "n5": (("grid", 70, 15), 0.62, (160, 120), 5, 64, "view", 0.0, 1),
    "sparse19": (("scattered", 300, 0), None, (160, 120), 19, 256, "view", 0.5, 1),
}
BOUND_CASES = [n for n in CASES if n not in ("s19",)]
TEXELS_PER_PIXEL = 1.5


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's scene: mesh, its eight ring cameras, the oracle's index planes of them (rendered once), P, C, views, seed."""
    from oracle import oracle
    from semantic_meshes_amd import data
    from test_gpu_compact_records import WIDE_SCALE, fine_grid, ring
    (kind, a, b), scale, size, C, views, fold_per, iew, group = CASES[name]
    if kind == "scattered":
        planes = scattered_planes(a, *size)
        return types.SimpleNamespace(name=name, mesh=None, cams=[None] * len(planes), planes=planes, P=a, C=C, views=views, size=size,
                                     fold_per=fold_per, iew=iew, group=group, texels=False, seed=sorted(CASES).index(name) + 100)
    mesh = fine_grid(a, b)
    if kind == "shuffled":
        perm = np.random.default_rng(6).permutation(len(mesh.faces))
        mesh = data.Mesh(mesh.vertices, np.asarray(mesh.faces)[perm])
    cams = ring(8, WIDE_SCALE if scale == "wide" else scale, *size)
    if kind == "texels":
        o = oracle.OracleRenderer(mesh.vertices, mesh.faces, cams, TEXELS_PER_PIXEL)
    else:
        o = oracle.OracleRenderer(mesh.vertices, mesh.faces)
    planes = [o.render(cam)[0] for cam in cams]
    return types.SimpleNamespace(name=name, mesh=mesh, cams=cams, planes=planes, P=o.getPrimitivesNum(), C=C, views=views, size=size,
                                 fold_per=fold_per, iew=iew, group=group, texels=kind == "texels", seed=sorted(CASES).index(name) + 100)


# image_records.hip: a primitive whose pixels fit no 8 x 8 box and whose bounding box holds more than 16 n + 256 pixels is "sparse" --
# not for the triangle-order kernels: its terms go through float64 atomics (k_scatter_sparse) and are folded by k_fold_sparse
SPARSE_FACTOR, SPARSE_SLACK = 16, 256


def box_areas(plane, P):
    """(n, area) per primitive of an index plane: its pixels and the pixels of their bounding box."""
    W, H = plane.shape
    xs, ys = np.nonzero(plane < P)
    v = plane[xs, ys].astype(np.int64)
    n = np.bincount(v, minlength=P)
    x0, y0 = np.full(P, W), np.full(P, H)
    x1, y1 = np.full(P, -1), np.full(P, -1)
    np.minimum.at(x0, v, xs), np.minimum.at(y0, v, ys), np.maximum.at(x1, v, xs), np.maximum.at(y1, v, ys)
    return n, np.where(n > 0, (x1 - x0 + 1) * (y1 - y0 + 1), 0)


def scattered_planes(P, W, H, planes=8):
    """Index images no renderer made: every pixel draws its primitive at random (one pixel in ten is background), so a primitive's
    ~58 pixels lie all over the image -- every primitive is sparse, by a factor of ten and more."""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(planes):
        plane = rng.integers(0, P, (W, H)).astype(np.uint32)
        plane[rng.random((W, H)) < 0.1] = np.uint32(0xFFFFFFFF)
        n, area = box_areas(plane, P)
        assert (n > 8).all() and (area > 10 * (SPARSE_FACTOR * n + SPARSE_SLACK)).all()
        out.append(plane)
    return out


# ---- non-finite members over a run (case "n5": C = 5, iew = 0, one view per call, weights in every other view) ------------------
# role: (view of the edit, what is written into one pixel of the row)
NONFINITE_ROLES = ("wiped", "emptied", "negative", "infinite", "unweighted")


@functools.lru_cache(maxsize=None)
def nonfinite_rows(name="n5"):
    """{role: row}: five rows that every camera sees (so every view folds them), far apart."""
    cs = case(name)
    seen = np.ones(cs.P, bool)
    for pl in cs.planes:
        seen &= np.bincount(pl[pl < cs.P].astype(np.int64), minlength=cs.P) > 0
    rows = np.nonzero(seen)[0]
    assert len(rows) >= 50
    return dict(zip(NONFINITE_ROLES, (int(r) for r in rows[np.linspace(5, len(rows) - 5, 5).astype(int)])))


def nonfinite_edits(cs, i, probs, weights):
    """The edits of view i, in place.  "wiped": p = 0 in class 2 in view 3.  "emptied": p = 0 in class c in view 10 + 6 c.  "negative":
    p = -0.25 in class 1 in view 4.  "infinite": p = +inf in class 0 in view 6.  "unweighted": p = 0 in class 3 under a zero weight in
    view 7 (nothing is added).  The edited pixel is the row's first in the view, its other classes 0.3 (it contributes: sum > 0.5)."""
    rows = nonfinite_rows(cs.name)
    plane = cs.planes[i % len(cs.cams)]

    def pixel(role):
        xs, ys = np.nonzero(plane == rows[role])
        return int(xs[0]), int(ys[0])

    def write(role, c, value):
        x, y = pixel(role)
        probs[x, y, :] = F32(0.3)
        probs[x, y, c] = F32(value)
        return x, y
    if i == 3:
        write("wiped", 2, 0.0)
    if i >= 10 and (i - 10) % 6 == 0 and (i - 10) // 6 < cs.C:
        write("emptied", (i - 10) // 6, 0.0)
    if i == 4:
        write("negative", 1, -0.25)
    if i == 6:
        write("infinite", 0, np.inf)
    if i == 7:
        x, y = write("unweighted", 3, 0.0)
        assert weights is not None
        weights[x, y] = F32(0)
