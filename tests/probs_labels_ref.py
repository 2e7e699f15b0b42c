"""numpy model of include/smesh_probs_labels.h for the tests: the rule as an explicit class loop (vectorised over pixels, float32
running sum), the same rule for ONE row in plain Python, the planted rows that exercise every clause of it, and the test images."""
import numpy as np

import half_helpers as hh

DTYPES = ("float32", "float16", "bfloat16")
LBL_DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64")


def ref_labels(rows, threshold=None):
    """(labels int64, don't care bool) of float32 class vectors `rows` [..., C]: best = r[0], label = 0; ascending c: r[c] > best
    replaces.  t = the float32 sum in ascending class order from 0.0f; don't care iff t < threshold (None: no test)."""
    r = np.asarray(rows)
    assert r.dtype == np.float32 and r.shape[-1] >= 1
    best = r[..., 0].copy()
    label = np.zeros(r.shape[:-1], np.int64)
    t = np.zeros(r.shape[:-1], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = t + r[..., 0]
        for c in range(1, r.shape[-1]):
            v = r[..., c]
            t = t + v
            m = v > best
            best = np.where(m, v, best)
            label = np.where(m, c, label)
        assert t.dtype == np.float32
        dc = np.zeros(label.shape, bool) if threshold is None else t < np.float32(threshold)
    return label, dc


def row_label(row, threshold=None):
    """The rule for one row, element by element in Python (np.float32 scalars): (label, don't care)."""
    row = [np.float32(v) for v in row]
    best, label, t = row[0], 0, np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(t + row[0])
        for c in range(1, len(row)):
            t = np.float32(t + row[c])
            if row[c] > best:
                best, label = row[c], c
        return label, (threshold is not None and bool(t < np.float32(threshold)))


def planted_rows(C):
    """[(name, float32 row [C])]: every clause of the rule.  All values are exact in bfloat16 and float16 alike (small dyadic numbers,
    multiples of 2^-24 up to 13 for the subnormals), so a narrowed image holds the same rows.  Cases that need more classes than C
    are left out."""
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    out = []

    def base(v=0.125):
        return np.full(C, v, f)

    if C >= 2:
        r = base(); r[C // 3] = 0.75; r[C - 1] = 0.75                   # the maximum at two classes: the lower one wins
        out.append(("duplicate maximum", r))
        r = base(-1.0); r[0] = -0.0; r[1] = 0.0                         # -0 first, +0 later: equal, class 0 stays
        out.append(("-0 then +0", r))
        r = base(-1.0); r[0] = 0.0; r[1] = -0.0
        out.append(("+0 then -0", r))
        r = base(); r[C - 1] = inf
        out.append(("+inf", r))
        r = base(-2.0); r[0] = -inf; r[C - 1] = -1.5
        out.append(("-inf at r[0]", r))
        r = base(); r[0] = nan; r[C - 1] = 0.75                          # a NaN r[0] is never replaced
        out.append(("NaN at r[0]", r))
        r = base(); r[1] = nan; r[0] = 0.5                               # a NaN never replaces the best
        out.append(("NaN later, best before", r))
    if C >= 3:
        r = base(); r[1] = nan; r[C - 1] = 0.75
        out.append(("NaN later, best after", r))
        r = base(); r[0] = -inf; r[1] = -inf; r[2] = -inf                # -inf everywhere it can be: still ordinary values
        out.append(("-inf ties", r))
    out.append(("all equal", base(0.25)))
    out.append(("all negative", np.array([-(1 + ((5 * c + 3) % 7)) * 0.25 for c in range(C)], f)))
    out.append(("float16 subnormals", np.array([((7 * c + 4) % 13 + 1) * 2.0 ** -24 for c in range(C)], f)))
    return out


def is_planted(name, row):
    """Does `row` (float32, after any narrowing and widening) still show the case `name`?"""
    C = len(row)
    with np.errstate(invalid="ignore"):
        if name == "duplicate maximum":
            return row[C // 3] == row[C - 1] == np.nanmax(row) and C // 3 != C - 1
        if name == "-0 then +0":
            return row[0] == 0 and np.signbit(row[0]) and row[1] == 0 and not np.signbit(row[1]) and (row[2:] < 0).all()
        if name == "+0 then -0":
            return row[0] == 0 and not np.signbit(row[0]) and row[1] == 0 and np.signbit(row[1]) and (row[2:] < 0).all()
        if name == "+inf":
            return row[C - 1] == np.inf
        if name == "-inf at r[0]":
            return row[0] == -np.inf and np.isfinite(row[1:]).all()
        if name == "NaN at r[0]":
            return np.isnan(row[0]) and not np.isnan(row[1:]).any()
        if name.startswith("NaN later"):
            return np.isnan(row[1]) and not np.isnan(row[0])
        if name == "-inf ties":
            return (row[:3] == -np.inf).all()
        if name == "all equal":
            return (row == row[0]).all()
        if name == "all negative":
            return (row < 0).all()
        if name == "float16 subnormals":
            return ((row > 0) & (row < 2.0 ** -14)).all()
    raise KeyError(name)


def make_probs(rng, W, H, C, dtype):
    """(values, widened, planted): `values` (W,H,C) is what a user hands over -- float32, float16, or uint16 bits of bfloat16;
    `widened` its exact float32 image; `planted` [(name, x, y)].  Seeded softmax rows, about a third of them scaled by a half (their
    sum falls below 0.9), with the rows of planted_rows written into the first pixels in (x, y) order, as many as fit."""
    logits = rng.normal(0.0, 3.0, size=(W, H, C)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    p = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    p[rng.random((W, H)) < 1.0 / 3.0] *= np.float32(0.5)
    planted = []
    for k, (name, row) in enumerate(planted_rows(C)):
        if k >= W * H:
            break
        p[k // H, k % H] = row
        planted.append((name, k // H, k % H))
    if dtype == "float32":
        return p, p, planted
    bits = hh.narrow(p, dtype)
    return hh.typed(bits, dtype), hh.widen(bits, dtype), planted


def one_hot(labels, C):
    """tf.one_hot: a label outside [0, C) is the all-zero vector."""
    lab = np.asarray(labels).astype(np.int64)
    return ((lab[..., None] == np.arange(C)) & (lab[..., None] >= 0)).astype(np.float32)


def expected_matrix(pred, gt, C):
    """(M uint64 [C, C + 1], ignored) of int predictions and ground truth of any shape; predictions outside [0, C) are don't care."""
    pred = np.asarray(pred).astype(np.int64).ravel()
    g = np.asarray(gt)
    g = (g.astype(np.int64) if g.dtype != np.uint64 else np.where(g < 2 ** 62, g, 2 ** 62).astype(np.int64)).ravel()
    ok = (g >= 0) & (g < C)
    p = np.where((pred >= 0) & (pred < C), pred, C)
    M = np.zeros((C, C + 1), np.uint64)
    np.add.at(M, (g[ok], p[ok]), 1)
    return M, int((~ok).sum())


def make_gt(rng, shape, C, dtype):
    """Ground truth of `dtype`: classes in [0, C), about 3 % out of range (C, C + 7, the dtype's maximum; negative values for the
    signed dtypes).  Values the dtype cannot hold wrap -- the expectation is computed from the typed array."""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    g = rng.integers(0, C, size=shape).astype(np.int64)
    bad_values = [C, C + 7, min(int(info.max), 2 ** 62)] + ([-1, -C - 1, int(info.min)] if dt.kind == "i" else [])
    bad = rng.random(shape) < 0.03
    out = np.where(bad, rng.choice(np.array(bad_values, np.int64), size=shape), g).astype(dt)
    if dt == np.uint64:
        out[out == 2 ** 62] = info.max
    return out
