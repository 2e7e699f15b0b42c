"""The closest face of a point (include/smesh_points.h) in numpy: the header's rule operation by operation, elementwise and broadcast
[N,1,3] against [1,F,3], every sum parenthesised as written.  The cases are applied with np.where in REVERSE order, so that case 1 has
the last word, and the minimum is taken lexicographically by (dist2, f).  The same functions take np.float64.

This is the reference of every comparison in tests/test_points_host.py and tests/test_gpu_points.py; it is never the code under test."""
import numpy as np


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def dist2_all(vertices, faces, points, dtype=np.float32):
    """[N,F] dist2(q, f) in `dtype`.  NaN where the rule gives NaN."""
    v = np.asarray(vertices, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    q = np.asarray(points, dtype).reshape(-1, 1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = q - a, q - b, q - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        one, zero = dtype(1), dtype(0)
        den = one / ((va + vb) + vc)
        r = (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]                                   # 7
        t6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        r = np.where(((va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero))[..., None], b + t6[..., None] * bc, r)   # 6
        t5 = d2 / (d2 - d6)
        r = np.where(((vb <= zero) & (d2 >= zero) & (d6 <= zero))[..., None], a + t5[..., None] * ac, r)                 # 5
        r = np.where(((d6 >= zero) & (d5 <= d6))[..., None], c, r)                                                       # 4
        t3 = d1 / (d1 - d3)
        r = np.where(((vc <= zero) & (d1 >= zero) & (d3 <= zero))[..., None], a + t3[..., None] * ab, r)                 # 3
        r = np.where(((d3 >= zero) & (d4 <= d3))[..., None], b, r)                                                       # 2
        r = np.where(((d1 <= zero) & (d2 <= zero))[..., None], a, r)                                                     # 1
        e = q - r
        out = _dot(e, e)
    assert out.dtype == dtype
    return out


def nearest(vertices, faces, points, max_distance=None, dtype=np.float32, chunk=256):
    """(faces int32 [N], dist2 `dtype` [N]): the exhaustive scan.  A candidate replaces the best when dist2 < best, or dist2 == best
    and f < best_f, from (+inf, -1): NaN and +inf never win.  With max_distance R, a best that does not satisfy dist2 <= R * R (in
    `dtype`) becomes (-1, +inf); so does a point with a non-finite coordinate."""
    pts = np.asarray(points, dtype).reshape(-1, 3)
    N, F = len(pts), len(np.asarray(faces).reshape(-1, 3))
    out_f, out_d = np.full(N, -1, np.int32), np.full(N, np.inf, dtype)
    if F == 0 or N == 0:
        return out_f, out_d
    for lo in range(0, N, chunk):
        d = dist2_all(vertices, faces, pts[lo:lo + chunk], dtype)
        d = np.where(np.isnan(d), dtype(np.inf), d)
        best = d.min(axis=1)
        first = np.argmax(d == best[:, None], axis=1)           # the lowest f among equal values
        win = np.isfinite(best)
        out_f[lo:lo + chunk] = np.where(win, first, -1)
        out_d[lo:lo + chunk] = np.where(win, best, dtype(np.inf))
    bad = ~np.isfinite(pts).all(axis=1)
    if max_distance is not None:
        r2 = dtype(max_distance) * dtype(max_distance)
        bad |= ~(out_d <= r2)
    out_f[bad], out_d[bad] = -1, np.inf
    return out_f, out_d


def soup(seed=1, F=512, N=1024, extent=0.3):
    """The seeded random soup of the tests: F triangles with centres uniform in the unit cube and vertices drawn as
    centre + extent * (U - 0.5), N points uniform in [-0.2, 1.2]^3.  (vertices float32 [3F,3], faces int32 [F,3], points float32 [N,3])"""
    rng = np.random.default_rng(seed)
    centres = rng.random((F, 1, 3))
    vertices = (centres + extent * (rng.random((F, 3, 3)) - 0.5)).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    points = (-0.2 + 1.4 * rng.random((N, 3))).astype(np.float32)
    return vertices, faces, points
