"""The numpy restatement of include/smesh_face_graph.h that the host and the GPU tests compare against: the face graph, the
propagation and the normal weights, each by the header's rule and by a route that is not the library's.

  adjacency   the library walks vertex-to-faces lists per face; here the unordered edge keys of all faces are sorted and grouped,
              and every face and slot emits its group less itself, in ascending face order.
  propagate   float32 arrays; the j-th informed entry of EVERY face is added in one vectorised step, for j = 0, 1, ..., so each
              face's additions happen in list order, one float32 operation after another (numpy never fuses a product and a sum).
  weights     the header's operations, one numpy float32 operation each."""
import numpy as np

SMOOTH, FILL = 0, 1


def edge_slots(faces, V):
    """(key int64[F,3], valid bool[F,3]): the unordered-pair key of every edge slot, and False where the slot is skipped (two equal
    vertices, or the pair of an earlier slot of the same face)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f, f[:, [1, 2, 0]]
    key = np.minimum(a, b) * max(int(V), 1) + np.maximum(a, b)
    valid = a != b
    valid[:, 1] &= key[:, 1] != key[:, 0]
    valid[:, 2] &= (key[:, 2] != key[:, 0]) & (key[:, 2] != key[:, 1])
    return key, valid


def adjacency(faces, V):
    """(offsets uint64[F+1], neighbours uint32[nnz])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    key, valid = edge_slots(f, V)
    slot_face = np.repeat(np.arange(F, dtype=np.int64), 3)[valid.ravel()]      # the valid slots in (face, slot) order
    slot_key = key.ravel()[valid.ravel()]
    # the faces of every key, ascending: sort by (key, face); a face holds a key at most once (the second time is skipped)
    order = np.lexsort((slot_face, slot_key))
    skey, sface = slot_key[order], slot_face[order]
    uniq, start, count = np.unique(skey, return_index=True, return_counts=True)
    group = np.searchsorted(uniq, slot_key)                                    # the group of every slot
    n = count[group]                                                           # candidates per slot (itself included)
    first = np.cumsum(n) - n
    slot_of = np.repeat(np.arange(len(n)), n)
    cand = sface[np.repeat(start[group], n) + (np.arange(int(n.sum())) - np.repeat(first, n))]
    keep = cand != slot_face[slot_of]
    neighbours = cand[keep].astype(np.uint32)
    per_face = np.bincount(slot_face[slot_of][keep], minlength=F)
    offsets = np.zeros(F + 1, np.uint64)
    offsets[1:] = np.cumsum(per_face)
    return offsets, neighbours


def row_totals(x):
    """float32 [F]: the sum of every row in ascending c, from 0."""
    t = np.zeros(x.shape[0], np.float32)
    for c in range(x.shape[1]):
        t = t + x[:, c]
    return t


def propagate(offsets, neighbours, x0, iterations, mode, alpha=0.5, observed_threshold=0.9, weights=None, trace=None):
    """(x_T float32[F,C], tot_T float32[F]).  `trace`: a list that receives, per iteration, the masks (kept, averaged, stayed) of
    the three FILL branches (SMOOTH: kept is empty, stayed = no informed neighbour)."""
    x0 = np.ascontiguousarray(x0, np.float32)
    F, C = x0.shape
    off = np.asarray(offsets).astype(np.int64)
    nbr = np.asarray(neighbours).astype(np.int64)
    deg = np.diff(off)
    face_of = np.repeat(np.arange(F, dtype=np.int64), deg)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    alpha = np.float32(alpha)
    om = np.float32(1.0) - alpha
    thr = np.float32(observed_threshold)
    x, tot = x0, row_totals(x0)
    tot0 = tot
    for _ in range(int(iterations)):
        informed = tot[nbr] > 0
        idx = np.flatnonzero(informed)                                         # informed entries, in CSR order
        fo = face_of[idx]
        before = np.concatenate([[0], np.cumsum(informed)])                    # informed entries before entry k, over the whole array
        rank = before[idx] - before[off[:-1]][fo]                              # ... and within the entry's own face
        s = np.zeros((F, C), np.float32)
        d = np.zeros(F, np.float32)
        n = np.zeros(F, np.int64)
        for j in range(int(rank.max()) + 1 if len(idx) else 0):
            sel = idx[rank == j]
            fs = face_of[sel]                                                  # (distinct: one j-th informed entry per face)
            if w is None:
                s[fs] = s[fs] + x[nbr[sel]]
                n[fs] += 1
            else:
                s[fs] = s[fs] + w[sel][:, None] * x[nbr[sel]]
                d[fs] = d[fs] + w[sel]
        if w is None:
            d = n.astype(np.float32)
        has = d > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s / d[:, None]
        if mode == SMOOTH:
            new = np.where(has[:, None], om * x0 + alpha * m, x0).astype(np.float32)
            kept = np.zeros(F, bool)
        else:
            kept = tot0 >= thr
            new = np.where(kept[:, None], x0, np.where(has[:, None], m, x)).astype(np.float32)
        if trace is not None:
            trace.append((kept, ~kept & has, ~kept & ~has))
        x, tot = new, row_totals(new)
    return x, tot


def finish(x, tot, threshold):
    """(labels int32[F], don't-care mask, unreached): the finishing step of smesh_vertices.h on x_T."""
    dc = tot < np.float32(threshold)
    labels = np.argmax(x, axis=1).astype(np.int32) if x.shape[1] else np.zeros(len(x), np.int32)
    labels[dc] = -1
    return labels, dc, int((~(tot > 0)).sum())


def normals(vertices, faces):
    """(n float32[F,3], l float32[F])."""
    v = np.ascontiguousarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
    n = np.stack([nx, ny, nz], axis=1)
    assert n.dtype == np.float32 and l.dtype == np.float32
    return n, l


def normal_weights(offsets, neighbours, vertices, faces, power=4, two_sided=True):
    """float32 [nnz]."""
    n, l = normals(vertices, faces)
    off = np.asarray(offsets).astype(np.int64)
    g = np.asarray(neighbours).astype(np.int64)
    f = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    with np.errstate(all="ignore"):
        q = ((n[f, 0] * n[g, 0] + n[f, 1] * n[g, 1]) + n[f, 2] * n[g, 2]) / (l[f] * l[g])
        if two_sided:
            q = np.abs(q)
        q = np.where(q > 0, q, np.float32(0)).astype(np.float32)
        q = np.where(q > 1, np.float32(1), q).astype(np.float32)
        p = q
        for _ in range(int(power) - 1):
            p = p * q
    assert p.dtype == np.float32
    return p
