"""The restatement of include/smesh_segment_stats.h that the host and the GPU tests compare against, by another route than the
library's: the library sorts the labelled faces by one stable split per bit of the segment id and gives every chunk of 256 members
to a group of lanes; here `np.argsort(ids, kind="stable")` gives the members, the chunk sums run as 256 vectorised steps across all
chunks at once, and the pooled rows as one vectorised step per chunk index across all segments.  Every addition and multiplication
is one explicit float32 operation on float32 arrays; nothing goes through np.sum or np.add.reduce, which add pairwise."""
import numpy as np

import face_graph_ref

CHUNK = 256
SUMS, ANNOTATIONS = 0, 1                          # SMESH_VTX_*


def members(ids, count):
    """(offsets uint32[count+1], members uint32[labelled]): the faces of every segment, ascending, back to back."""
    ids = np.asarray(ids, np.int64)
    order = np.argsort(ids, kind="stable")        # the unlabelled faces (-1) first, then segment after segment, ascending within
    labelled = int((ids >= 0).sum())
    size = np.bincount(ids[ids >= 0], minlength=count)
    assert len(size) == count
    offsets = np.zeros(count + 1, np.uint32)
    offsets[1:] = np.cumsum(size)
    return offsets, order[len(ids) - labelled:].astype(np.uint32)


def pooled(rows, ids, count, weights=None):
    """float32 [count,C]: the header's `pooled`."""
    rows = np.ascontiguousarray(rows, np.float32)
    C = rows.shape[1]
    offsets, mem = members(ids, count)
    offsets, mem = offsets.astype(np.int64), mem.astype(np.int64)
    size = np.diff(offsets)
    term = rows[mem]
    if weights is not None:
        w = np.ascontiguousarray(weights, np.float32)
        assert w.shape == (len(rows),)
        with np.errstate(all="ignore"):
            term = w[mem][:, None] * term          # one multiplication
    assert term.dtype == np.float32
    chunks = (size + CHUNK - 1) // CHUNK
    start = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
    seg = np.repeat(np.arange(count, dtype=np.int64), chunks)
    k = np.arange(int(start[-1]), dtype=np.int64) - start[seg]
    begin = offsets[seg] + CHUNK * k
    n = np.minimum(CHUNK, size[seg] - CHUNK * k)
    p = np.zeros((len(seg), C), np.float32)
    with np.errstate(all="ignore"):
        for r in range(CHUNK):                     # rank r of every chunk that has one
            sel = np.flatnonzero(n > r)
            if not len(sel):
                break
            p[sel] = p[sel] + term[begin[sel] + r]
        out = np.zeros((count, C), np.float32)
        for j in range(int(chunks.max()) if count else 0):      # chunk j of every segment that has one
            sel = np.flatnonzero(chunks > j)
            out[sel] = out[sel] + p[start[sel] + j]
    assert p.dtype == np.float32 and out.dtype == np.float32
    return out


def finish(x, mode, threshold):
    """(rows float32[n,C], labels int32[n]): the finishing step of smesh_vertices.h on every row of x."""
    x = np.ascontiguousarray(x, np.float32)
    tot = face_graph_ref.row_totals(x)
    labels, dont_care, _ = face_graph_ref.finish(x, tot, threshold)
    if mode == SUMS:
        return x.copy(), labels
    with np.errstate(all="ignore"):
        out = (x / tot[:, None]).astype(np.float32)
    out[dont_care] = np.float32(0.0)
    return out, labels


def pooled_faces(rows, ids, count, weights=None):
    """float32 [F,C]: the header's face form X, before its finish."""
    rows = np.ascontiguousarray(rows, np.float32)
    ids = np.asarray(ids, np.int64)
    x = rows.copy()
    x[ids >= 0] = pooled(rows, ids, count, weights)[ids[ids >= 0]]
    return x


def face_areas(vertices, faces):
    """float32 [F]."""
    n, l = face_graph_ref.normals(vertices, faces)
    area = np.float32(0.5) * l
    assert area.dtype == np.float32
    return area


def areas(face_area, ids, count):
    """float32 [count]."""
    return pooled(np.ascontiguousarray(face_area, np.float32)[:, None], ids, count)[:, 0]


def kept(ids, measure, minimum):
    """bool [F]: labelled, and measure[ids[f]] >= minimum (false for a NaN on either side)."""
    ids = np.asarray(ids, np.int64)
    out = np.zeros(len(ids), bool)
    with np.errstate(invalid="ignore"):
        out[ids >= 0] = np.asarray(measure, np.float32)[ids[ids >= 0]] >= np.float32(minimum)
    return out


def despeckle_labels_by(labels, ids, measure, minimum):
    """(labels int32[F] with every face that is not kept at -1, removed faces, removed segments)."""
    lab = np.asarray(labels)
    k = kept(ids, measure, minimum)
    with np.errstate(invalid="ignore"):
        failing = int((~(np.asarray(measure, np.float32) >= np.float32(minimum))).sum())
    return np.where(k, lab, -1).astype(np.int32), int(((lab >= 0) & ~k).sum()), failing


def despeckle_rows_by(rows, ids, measure, minimum):
    """float32 [F,C]: `rows` with +0.0 in every class of a face that is labelled and not kept."""
    out = np.array(rows, np.float32, copy=True)
    out[(np.asarray(ids) >= 0) & ~kept(ids, measure, minimum)] = np.float32(0.0)
    return out
