"""The restatement of include/smesh_face_segments.h that the host and the GPU tests compare against, by another route than the
library's: the library runs a lock-free union-find and numbers its roots with a scan; here every face in ASCENDING order that has
no segment yet starts the next one, and a breadth-first flood fill over the links, taken in both directions, gives it its faces.
Ascending starts make the numbering the header's (segments in the order of their lowest face) without any sorting.  Plain Python
over numpy arrays; no union-find, no scipy."""
from collections import deque

import numpy as np

import face_graph_ref


def link_mask(offsets, neighbours, labels, weights=None, min_weight=None):
    """bool [nnz]: does entry k of its face link the two faces it names?"""
    off = np.asarray(offsets).astype(np.int64)
    g = np.asarray(neighbours).astype(np.int64)
    lab = np.asarray(labels).astype(np.int64)
    f = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    ok = (lab[f] >= 0) & (lab[f] == lab[g])
    if weights is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(weights, np.float32) >= np.float32(min_weight)      # (False for a NaN)
    return f, g, ok


def segments(offsets, neighbours, labels, weights=None, min_weight=None):
    """(ids int32[F], first_face uint32[S], label int32[S], size uint32[S])."""
    lab = np.asarray(labels)
    F = len(lab)
    f, g, ok = link_mask(offsets, neighbours, labels, weights, min_weight)
    # links are undirected: every linking entry in both directions, grouped by its first face
    a, b = np.concatenate([f[ok], g[ok]]), np.concatenate([g[ok], f[ok]])
    order = np.argsort(a, kind="stable")
    b = b[order].tolist()
    start = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=F))]).tolist()
    ids = [-1] * F
    labelled = (lab >= 0).tolist()
    first_face, size = [], []
    for seed in range(F):
        if not labelled[seed] or ids[seed] >= 0:
            continue
        s = len(first_face)
        ids[seed] = s
        n = 1
        queue = deque([seed])
        while queue:
            x = queue.popleft()
            for y in b[start[x]:start[x + 1]]:
                if ids[y] < 0:
                    ids[y] = s
                    n += 1
                    queue.append(y)
        first_face.append(seed)
        size.append(n)
    first_face = np.asarray(first_face, np.uint32)
    return (np.asarray(ids, np.int32), first_face, lab[first_face.astype(np.int64)].astype(np.int32), np.asarray(size, np.uint32))


def kept(labels, ids, size, min_faces):
    """bool [F]: labelled, and in a segment of at least `min_faces` faces."""
    lab = np.asarray(labels)
    out = np.zeros(len(lab), bool)
    sel = lab >= 0
    out[sel] = np.asarray(size).astype(np.int64)[ids[sel]] >= int(min_faces)
    return out


def despeckle_labels(labels, ids, size, min_faces):
    """(labels int32[F] with every face that is not kept at -1, removed faces, removed segments)."""
    lab = np.asarray(labels)
    k = kept(lab, ids, size, min_faces)
    out = np.where(k, lab, -1).astype(np.int32)
    return out, int(((lab >= 0) & ~k).sum()), int((np.asarray(size).astype(np.int64) < int(min_faces)).sum())


def despeckle_rows(rows, labels, ids, size, min_faces):
    """float32 [F,C]: `rows` with +0.0 in every class of a face that is labelled and not kept."""
    lab = np.asarray(labels)
    out = np.array(rows, np.float32, copy=True)
    out[(lab >= 0) & ~kept(lab, ids, size, min_faces)] = np.float32(0.0)
    return out


def row_labels(rows, threshold):
    """int32 [F]: the finishing step of smesh_vertices.h on every row (argmax, the lowest class among equals, -1 below the threshold)."""
    rows = np.ascontiguousarray(rows, np.float32)
    return face_graph_ref.finish(rows, face_graph_ref.row_totals(rows), threshold)[0]
