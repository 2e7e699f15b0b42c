"""The cases of tests/mesh_graph_scale_cases.py are what they are for -- on the references alone, without a GPU: every size lies on
the intended side of the two launch thresholds, and every label pattern has the structure that makes it worth its time."""
import numpy as np

import face_segments_ref as sref
import mesh_graph_scale_cases as cases

SCAN_CHUNK = 256 * 1024          # kBlock * kScanTile (scan.inc.hpp): k_scan_sums takes a second chunk, and its carry, beyond this
CAPPED_GRID = 2048 * 256         # kCountBlocks * kBlock (face_segments.hip): a lane of the capped grid takes a second item beyond this


def test_every_size_lies_on_its_side_of_the_thresholds():
    assert (cases.SCAN_CHUNK, cases.CAPPED_GRID) == (SCAN_CHUNK, CAPPED_GRID)
    faces, vertices, V, offsets, nbr = cases.case("big")
    assert (len(faces), V, len(nbr)) == (530000, 266031, 1587940)
    assert len(faces) + 1 > CAPPED_GRID > SCAN_CHUNK
    assert -(-(len(faces) + 1) // 1024) == 518 and len(faces) + 1 - CAPPED_GRID == 5713      # scan tiles; items beyond the capped grid
    assert [F + 1 for F in cases.EDGE_FACES] == [262144, 262145, 524288, 524289]
    sides = []
    for F in cases.EDGE_FACES:
        sub = cases.case("first%d" % F)
        assert len(sub[0]) == F and sub[2] == V and np.array_equal(sub[0], faces[:F]) and len(sub[3]) == F + 1
        assert len(cases.labels("first%d" % F, "random2")) == F
        sides.append((F + 1 > SCAN_CHUNK, F + 1 > CAPPED_GRID))
    assert sides == [(False, False), (True, False), (True, False), (True, True)]
    # the vertex map scans V + 1 counts
    assert [v + 1 > SCAN_CHUNK for v in cases.VERTEX_COUNTS] == [False, True, True] and cases.VERTEX_COUNTS[0] + 1 == SCAN_CHUNK
    for v in cases.VERTEX_COUNTS:
        sub, nv = cases.vertex_case(v)
        assert nv == v and 500000 < len(sub) <= 530000 and sub.max() < v and np.array_equal(sub, faces[:len(sub)])
    assert len(cases.vertex_case(cases.VERTEX_COUNTS[2])[0]) == 530000


def test_the_shuffled_grid_is_the_big_grid_in_another_order():
    faces, vertices, V, offsets, nbr = cases.case("big")
    sfaces, _, sV, soffsets, snbr = cases.case("shuffled")
    perm, inverse = cases.permutation()
    assert sV == V and np.array_equal(sfaces, faces[perm]) and np.array_equal(np.sort(perm), np.arange(len(faces)))
    # not spatially coherent: neighbours in the face order are far apart on the grid
    assert np.median(np.abs(np.diff(perm))) > 100000
    # its own adjacency (recomputed for the permuted array) is the big grid's under the permutation: the list of face i is the list
    # of face perm[i], entry by entry (a slot of this mesh has at most one face across it), in the new numbering
    off, soff = offsets.astype(np.int64), soffsets.astype(np.int64)
    deg = np.diff(off)[perm]
    assert np.array_equal(np.diff(soff), deg) and len(snbr) == len(nbr)
    entry = np.repeat(off[perm], deg) + (np.arange(len(nbr)) - np.repeat(soff[:-1], deg))
    assert np.array_equal(snbr, inverse[nbr[entry]])
    assert np.abs(snbr.astype(np.int64) - np.repeat(np.arange(len(faces)), deg)).mean() > 100000


def test_the_patterns_are_what_they_are_for():
    F = 530000
    ids, first, label, size = cases.expected("big", "constant")
    assert len(first) == 1 and size[0] == F
    ids, first, label, size = cases.expected("big", "serpentine")
    assert (label == 1).sum() == 1 and size[label == 1][0] > 250000           # the corridor is one segment, half the mesh long
    ids, first, label, size = cases.expected("big", "blocks32_noisy")
    assert len(first) > 10000 and size.max() > 1000                           # the noise's islands, and the blocks they sit in
    ids, first, label, size = cases.expected("big", "random2")
    lab = cases.labels("big", "random2")
    assert 0.08 < (lab < 0).mean() < 0.12 and set(np.unique(lab).tolist()) == {-1, 0, 1}
    assert 1000 < len(first) and size.max() < 5000                            # thousands of segments, none over a few thousand faces
    assert int(size.sum()) == int((lab >= 0).sum())
    # the shuffled grid carries the same labels on the same triangles: the same segments as sets of triangles
    perm, inverse = cases.permutation()
    for pattern in ("constant", "blocks32_noisy"):
        assert np.array_equal(cases.labels("shuffled", pattern), cases.labels("big", pattern)[perm])
        big, shuffled = cases.expected("big", pattern), cases.expected("shuffled", pattern)
        assert len(big[1]) == len(shuffled[1]) and np.array_equal(np.sort(big[3]), np.sort(shuffled[3]))
        # one segment of the big grid <-> one of the shuffled: the pairs (id there, id here) of all faces are as many as the segments
        pairs = np.unique(np.stack([big[0][perm], shuffled[0]]), axis=1)
        assert pairs.shape[1] == len(big[1]) + (1 if (big[0] < 0).any() else 0)


def test_the_isolated_triangles_give_more_segments_than_the_capped_grid_has_lanes():
    faces, vertices, V, offsets, nbr = cases.case("isolated")
    assert len(nbr) == 0 and not offsets.any() and V == 3 * len(faces)
    for pattern, want in (("constant", 530000), ("seventh", 530000 - 75715)):
        lab = cases.labels("isolated", pattern)
        ids, first, label, size = cases.expected("isolated", pattern)
        num_labelled = int((lab >= 0).sum())
        assert len(first) == num_labelled == want and (size == 1).all()
        # constant: more SEGMENTS than lanes, the strided turn of k_seg_small; every seventh at -1 leaves 454 285, which numbers the
        # segments past unlabelled faces while the faces are still more than the lanes
        assert (num_labelled > CAPPED_GRID) == (pattern == "constant") and len(lab) > CAPPED_GRID
        assert np.array_equal(ids, np.where(lab >= 0, np.cumsum(lab >= 0) - 1, -1))      # a running count of the labelled faces


def test_the_weights_and_rows_are_what_they_are_for():
    faces, vertices, V, offsets, nbr = cases.case("big")
    w, min_weight = cases.entry_weights("big", "asymmetric")
    f, g, ok = sref.link_mask(offsets, nbr, cases.labels("big", "blocks32_noisy"), w, min_weight)
    # entries that pass towards a HIGHER face while the entry back fails: the links a hook that skipped g > f would lose
    passing = ok
    key = f * len(faces) + g
    order = np.argsort(key)
    back = order[np.searchsorted(key[order], g * len(faces) + f)]             # the entry of g's list that names f
    assert np.array_equal(f[back], g) and np.array_equal(g[back], f)
    assert int((passing & ~passing[back] & (g > f)).sum()) > 10000
    assert len(cases.expected("big", "blocks32_noisy", "asymmetric")[1]) > len(cases.expected("big", "blocks32_noisy")[1])
    w, min_weight = cases.entry_weights("big", "normal")
    assert w.dtype == np.float32 and len(w) == len(nbr) and (w <= 1).all() and (w >= min_weight).mean() > 0.9
    for C in (19, 40):
        x = cases.rows(C, C)
        tot = x.sum(axis=1)
        assert x.shape == (530000, C) and 0.29 < (tot == 0).mean() < 0.31 and 0.05 < ((tot > 0) & (tot < 0.5)).mean() < 0.15
