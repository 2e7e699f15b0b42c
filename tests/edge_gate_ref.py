"""numpy restatement of include/smesh_edge_gate.h: the occlusion-edge weights of one view and their counts, every arithmetic step a
single float32 IEEE operation in the header's order.  The window is taken by BRUTE FORCE -- one shifted copy of the plane per window
offset, (2 radius + 1)^2 of them -- so that it shares no structure with the separable kernel; `weights_separable` is the second,
separable form the host test holds it against.  Shared by test_edge_gate_host.py and test_gpu_edge_gate.py; nothing here calls the
product's library."""
import collections

import numpy as np

# radius: int 1 .. 8; abs_tol, rel_tol: float32; behind, front, silhouette: bool
Gate = collections.namedtuple("Gate", "radius abs_tol rel_tol behind front silhouette")

VISIBLE, BEHIND, FRONT, SILHOUETTE = 0, 1, 2, 3
MAX_RADIUS = 8


def gate(radius, abs_tol, rel_tol=0.0, behind=True, front=False, silhouette=False):
    """The gate of `fusion.EdgeGate(radius, abs_tol, rel_tol, behind, front, silhouette)`: the defaults of the Python layer, every
    number rounded to float32 once."""
    assert 1 <= int(radius) <= MAX_RADIUS
    return Gate(int(radius), np.float32(abs_tol), np.float32(rel_tol), bool(behind), bool(front), bool(silhouette))


def window(depth, radius):
    """(lo, hi, bg) of every pixel's window, brute force: lo / hi float32 (+inf / -inf where the window holds no finite depth), bg bool."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 2
    W, H = d.shape
    finite = np.isfinite(d)
    lo = np.full((W, H), np.inf, np.float32)
    hi = np.full((W, H), -np.inf, np.float32)
    bg = np.zeros((W, H), bool)
    for dx in range(-radius, radius + 1):
        for dy in range(-radius, radius + 1):
            # output pixels (X, Y) whose neighbour (X + dx, Y + dy) is inside the image
            x0, x1 = max(0, -dx), min(W, W - dx)
            y0, y1 = max(0, -dy), min(H, H - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            nb, ok = d[x0 + dx:x1 + dx, y0 + dy:y1 + dy], finite[x0 + dx:x1 + dx, y0 + dy:y1 + dy]
            out = (slice(x0, x1), slice(y0, y1))
            lo[out] = np.where(ok & (nb < lo[out]), nb, lo[out])
            hi[out] = np.where(ok & (nb > hi[out]), nb, hi[out])
            bg[out] |= ~ok
    return lo, hi, bg


def decide(depth, lo, hi, bg, g, weights_in=None):
    """Steps 1 .. 5 of the header from the window's lo, hi, bg: (weights float32 (W,H), counts uint64 [4])."""
    d = np.asarray(depth)
    w_in = np.ones(d.shape, np.float32) if weights_in is None else np.asarray(weights_in)
    assert w_in.dtype == np.float32 and w_in.shape == d.shape
    visible = np.isfinite(d)
    with np.errstate(invalid="ignore", over="ignore"):
        t = g.abs_tol + g.rel_tol * d                      # float32: a multiply, then an add
        assert t.dtype == np.float32
        behind = visible & g.behind & ((d - lo) > t)
        front = visible & ~behind & g.front & ((hi - d) > t)
    sil = visible & ~behind & ~front & g.silhouette & bg
    keep = visible & ~behind & ~front & ~sil
    w = np.where(keep, w_in, np.float32(0)).astype(np.float32)
    return w, np.array([visible.sum(), behind.sum(), front.sum(), sil.sum()], np.uint64)


def weights(depth, g, weights_in=None):
    """The rule: (weights float32 (W,H), counts uint64 [visible, behind, front, silhouette])."""
    lo, hi, bg = window(depth, g.radius)
    return decide(depth, lo, hi, bg, g, weights_in)


def window_separable(depth, radius):
    """`window` computed along y, then along x, from padded copies: the form the kernel takes (for the host test only)."""
    d = np.asarray(depth)
    W, H = d.shape
    r = radius
    finite = np.isfinite(d)
    dlo = np.pad(np.where(finite, d, np.float32(np.inf)), r, constant_values=np.inf)
    dhi = np.pad(np.where(finite, d, np.float32(-np.inf)), r, constant_values=-np.inf)
    dbg = np.pad(~finite, r, constant_values=False)
    ylo = np.min([dlo[:, k:k + H] for k in range(2 * r + 1)], axis=0)
    yhi = np.max([dhi[:, k:k + H] for k in range(2 * r + 1)], axis=0)
    ybg = np.any([dbg[:, k:k + H] for k in range(2 * r + 1)], axis=0)
    lo = np.min([ylo[k:k + W] for k in range(2 * r + 1)], axis=0)
    hi = np.max([yhi[k:k + W] for k in range(2 * r + 1)], axis=0)
    bg = np.any([ybg[k:k + W] for k in range(2 * r + 1)], axis=0)
    return lo.astype(np.float32), hi.astype(np.float32), bg


def weights_separable(depth, g, weights_in=None):
    lo, hi, bg = window_separable(depth, g.radius)
    return decide(depth, lo, hi, bg, g, weights_in)


def random_plane(rng, W, H, near=2.0, far=5.0, background=0.1):
    """A float32 (W,H) plane of two depth levels in blobs of a few pixels plus about `background` of +inf."""
    pick = rng.random((W, H))
    coarse = rng.random(((W + 3) // 4, (H + 3) // 4)) < 0.5
    level = np.kron(coarse, np.ones((4, 4), bool))[:W, :H]
    d = np.where(level, np.float32(near), np.float32(far)).astype(np.float32)
    d[pick < background] = np.inf
    return d
