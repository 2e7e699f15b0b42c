"""The cases of tests/image_kernels_scale_cases.py are what they are for -- on the references alone, without a GPU: every case lies
past the size at which its kernel's launch changes, and where a restatement has two forms they agree there."""
import numpy as np

import depth_gate_ref as dg
import edge_gate_ref as eg
import image_kernels_scale_cases as cases
import label_prep_ref as lp


def test_the_restated_constants():
    assert (cases.STAGE_WORDS, cases.PL_BLOCK, cases.GROUPS_PLAIN, cases.GROUPS_COUNT) == (6144, 256, 6, 4)
    assert (cases.CHUNK, cases.XCDS, cases.TILE_X, cases.TILE_Y, cases.MAX_GRID_Y, cases.NEAREST_64) == (4096, 8, 32, 64, 65535, 2 ** 32)
    assert [cases.pl_tile_pixels(C) for C in (3, 19, 23, 24, 40, 63, 150, 255)] == [256, 256, 256, 245, 149, 97, 40, 24]
    assert (cases.pl_cap(False), cases.pl_cap(True)) == (1536, 1024)


def test_every_probs_labels_case_has_three_rounds_and_a_partial_third():
    """work > 2 grid + grid / 4 at 256 CUs -- what the GPU test asserts from the launch's own report -- and work < 3 grid wherever a
    case has a shape of its own: only some workgroups do a third round, so the workgroups differ in their number of rounds."""
    seen = {}
    for name, (C, dtype, shape, layouts, counting) in cases.PL_CASES.items():
        cap = cases.pl_cap(counting)
        for layout in layouts:
            path, work = cases.pl_work(name, layout)
            assert path == ("tiled" if layout in cases.TILEABLE else "generic")
            assert work > 2 * cap + cap // 4, (name, layout, work, cap)
            if name != "generic3 counting":          # (it shares the plain case's image: every workgroup does three rounds, some four)
                assert work < 3 * cap, (name, layout, work, cap)
            assert shape[0] * shape[1] * C * (4 if dtype == "float32" else 2) < 100e6
            seen[(name, layout)] = work
    assert seen[("dense255", "dense")] == seen[("dense255", "offset")] == 3463 and 300 * 277 % 24 == 12
    assert seen[("rows255", "padded rows")] == seen[("rows255 permuted", "padded rows permuted")] == 720 * 5
    assert seen[("count63 float32", "dense")] == 2326 and seen[("dense19", "dense")] == 3461 and seen[("dense40", "dense")] == 3464
    assert seen[("generic3", "channel first")] == 3461
    # a workgroup's consecutive tiles of the padded rows: another place in the run, and a run whose base is aligned otherwise
    tiles_per_run, grid = 5, cases.pl_cap(False)
    assert grid % tiles_per_run != 0
    for itemsize in (4, 2):
        stride_bytes = (98 * 255 + 3) * itemsize
        bases = {((b + k * grid) // tiles_per_run * stride_bytes) % 16 for b in (0,) for k in range(3)}
        assert len(bases) == 3
    assert 98 == 4 * 24 + 2


def test_the_counting_cases_plant_what_the_matrix_must_show():
    for name in ("count63 float32", "generic3 counting"):
        C, dtype, shape, layouts, counting = cases.PL_CASES[name]
        for gdt in cases.COUNT_GT_DTYPES:
            gt = cases.pl_ground_truth(C, shape, gdt)
            assert gt.dtype == np.dtype(gdt) and (gt >= C).any() and (gt < C).mean() > 0.9
    M, ignored = cases.pl_matrix("generic3 counting", "uint8", 0.9)
    assert ignored > 0 and M[:, 3].sum() > 0 and int(M.sum()) + ignored == 1000 * 886


def test_the_planes_are_dealt_in_runs():
    assert [(cases.chunks(s), cases.xcd_grid(s), cases.per_xcd(s)) for s in cases.PLANES] == [(18, 24, 3), (9, 16, 2)]
    assert 283 * 251 == 71033 and 71033 % 4 == 1 and 211 * 173 == 36503
    for size in cases.PLANES:
        grid = cases.xcd_grid(size)
        dealt = [cases.xcd_chunk(b, grid) for b in range(grid)]
        assert sorted(dealt) == list(range(grid)) and dealt != list(range(grid))     # a permutation, and not the identity
    # what every shape of the sibling tests gives: one chunk per XCD, the identity
    for size in ((160, 120), (96, 64), (80, 56), (97, 61)):
        grid = cases.xcd_grid(size)
        assert cases.per_xcd(size) == 1 and [cases.xcd_chunk(b, grid) for b in range(grid)] == list(range(grid))
    # the group: the grid of the large view; the small view's two chunks go to workgroups 0 and 8, the other 22 return early
    large, small = cases.GROUP_SIZES
    grid = cases.xcd_grid(large)
    assert grid == 24 and cases.chunks(small) == 2
    assert [b for b in range(grid) if cases.xcd_chunk(b, grid) < cases.chunks(small)] == [0, 8]
    assert cases.GROUP_VIEWS == 9


def test_the_edge_views_have_unlike_tile_grids():
    a, b = (cases.tile_grid(s) for s in cases.EDGE_SIZES)
    assert (a, b) == ((2, 3), (4, 1)) and a[0] != b[0] and a[1] != b[1]
    assert cases.launch_tile_grid(cases.EDGE_SIZES) == (4, 3)
    widest = max(cases.EDGE_SIZES, key=lambda s: s[0])
    tallest = max(cases.EDGE_SIZES, key=lambda s: s[1])
    assert widest != tallest
    # a workgroup's tile is (blockIdx.x div rows of the LAUNCH, blockIdx.x mod them): decoded by a view's own rows the 4 x 1 view
    # would take workgroups 0 .. 3 for its four tiles, by the launch's it takes 0, 3, 6 and 9
    rows = cases.launch_tile_grid(cases.EDGE_SIZES)[1]
    assert [bx for bx in range(4 * rows) if bx % rows < b[1] and bx // rows < b[0]] == [0, 3, 6, 9]


def test_the_two_forms_of_the_edge_restatement_agree_at_these_sizes():
    for size in cases.EDGE_SIZES:
        depth, w_in = cases.edge_plane(size)
        # (on a plane of two levels every pixel near background is behind or in front first: the silhouette alone as well)
        for args in cases.EDGE_GATES + ((3, 0.15, 0.01, False, False, True),):
            g = eg.gate(*args)
            for weights in (None, w_in):
                brute, separable = eg.weights(depth, g, weights), eg.weights_separable(depth, g, weights)
                assert np.array_equal(brute[0].view(np.uint32), separable[0].view(np.uint32)) and np.array_equal(brute[1], separable[1])
                assert brute[1][eg.VISIBLE] > 0 and brute[1][1:].sum() > 0


def test_the_long_sides_cross_the_64_bit_threshold_and_the_references_are_exact_there():
    n, N = cases.LONG_SOURCE, cases.LONG_TARGET
    assert n > 32768 and N > 32768
    exact = [((2 * X + 1) * n) // (2 * N) for X in range(N)]                  # plain Python integers
    wide = [X for X in range(N) if (2 * X + 1) * n >= cases.NEAREST_64]
    assert wide and wide[0] == 53687 and wide[-1] == N - 1 and len(wide) < N   # pixels on either side of the threshold
    assert np.array_equal(lp.axis_index(n, N), exact) and np.array_equal(dg.axis_index(n, N), exact)
    assert lp.axis_index(n, N).dtype == np.int64 and exact[-1] == n - 1
    # a division of the product's low 32 bits gives another sample for every pixel beyond the threshold
    assert all(((2 * X + 1) * n % 2 ** 32) // (2 * N) != exact[X] for X in wide)
    assert np.array_equal(lp.axis_index(1, 1), [0])
    for axis in cases.LONG_AXES:
        assert cases.long_shape(N, axis)[axis] == N and cases.long_shape(N, axis)[1 - axis] == 1
        for C in cases.LONG_CLASSES:
            for with_map in (False, True):
                src, m, want = cases.long_labels(axis, C, with_map)
                assert src.shape == cases.long_shape(n, axis) and want.shape == cases.long_shape(N, axis)
                assert want.dtype == (np.uint8 if C <= 255 else np.uint16)
                # beyond the threshold most pixels carry a class (drawn independently from pixel to pixel), so a wrong index shows
                flat = want.reshape(-1).astype(np.int64)
                assert (flat[wide[0]:] != np.iinfo(want.dtype).max).mean() > 0.5
            img, colors, cls, want = cases.long_colors(axis, C)
            assert img.shape == cases.long_shape(n, axis) + (3,) and want.shape == cases.long_shape(N, axis)
        for dtype in (np.uint16, np.float32):
            depth, sensor, w_in, (want, counts) = cases.long_depth(axis, dtype)
            assert depth.shape == want.shape == cases.long_shape(N, axis) and sensor.shape == cases.long_shape(n, axis)
            assert counts[dg.VISIBLE] > 60000 and counts[dg.MISSING] > 3000 and counts[dg.INCONSISTENT] > 8000 and counts[dg.FAR] == 0
            kept = want.reshape(-1)[wide[0]:] != 0
            assert 0.5 < kept.mean() < 0.8


def test_the_wide_image_needs_a_second_turn_of_the_column_loop():
    (w, h), (W, H) = cases.WIDE_SOURCE, cases.WIDE_TARGET
    assert W == cases.MAX_GRID_Y + 1 == 65536
    assert [X for X in range(W) if X >= cases.MAX_GRID_Y] == [65535]           # the one column left to workgroup 0's second turn
    out = cases.wide_resized(8, "float32")
    assert out.shape == (W, H, 8) and out.dtype == np.float32
    # the last columns all sit on the source's last column (the clamp of the rule), so the last one equals its neighbours: the GPU
    # test hands the kernels an output filled with a value no result holds, and a column left out shows as that value
    assert np.array_equal(out[W - 1], out[W - 2]) and not np.array_equal(out[W - 1], out[0])
    assert np.isfinite(out).all() and (out >= 0).all() and (out < 1).all()
    for thr in cases.THRESHOLDS:
        lab, dc = cases.wide_labels("float32", thr)
        assert lab.shape == (W, H) and len(np.unique(lab)) > 5 and (thr is None or 0.1 < dc.mean() < 0.6)
