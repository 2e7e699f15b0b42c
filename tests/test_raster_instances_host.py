"""tests/raster_instances_cases.py checked on its own, without a GPU: the case tables reach every compiled instance of the rasteriser
or name it hook-only, every estimate keeps its margin from the thresholds, the restated launch shape gives what each case was built
for, and the decorated scene holds the boxes it claims, in the waves it claims."""
import ctypes

import numpy as np

import raster_instances_cases as rc


def test_the_case_tables_reach_every_instance():
    """Every instance the library can pick by itself is the restated dispatch of some case; the rest is reached under a hook."""
    seen = set()
    for name in rc.RENDER_CASES:
        seen |= rc.instances_of(rc.case_expectation("render", name))
    for name in rc.GROUP_CASES:
        seen |= rc.instances_of(rc.case_expectation("group", name))
    assert len(rc.ALL_INSTANCES) == 9 + 9 + 3 + 6 + 2 + 6
    assert rc.LIBRARY_INSTANCES - seen == set()
    assert seen & rc.HOOK_ONLY == set()
    hooked = set()
    for knob, (env, knobs, cases) in rc.HOOKS.items():
        got = set()
        for kind, name in cases:
            got |= rc.instances_of(rc.case_expectation(kind, name, knobs))
        assert rc.HOOK_INSTANCES.get(knob, set()) <= got
        hooked |= got
    assert rc.HOOK_ONLY <= hooked
    assert len(rc.HOOKS) <= 4
    # the hook-only launch shapes: a medium stage behind spread waves, one view and grouped; four groups of 64 triangles per wave
    both = [rc.case_expectation(kind, name, rc.HOOKS["spread balance"][1]) for kind, name in rc.HOOKS["spread balance"][2]]
    assert all(e["mode"] & 2 and e["stages"] & 2 for e in both) and {e["kernel"] for e in both} == {1, 2}
    assert all(rc.case_expectation(kind, name, rc.HOOKS["groups"][1])["groups"] == 4 for kind, name in rc.HOOKS["groups"][2])
    # ... none of which the library picks by itself
    for kind, table in (("render", rc.RENDER_CASES), ("group", rc.GROUP_CASES)):
        for name in table:
            e = rc.case_expectation(kind, name)
            assert e["groups"] == 1 and not (e["mode"] & 2 and e["stages"] & 2) and not (e["mode"] & 2 and e["kernel"] != 1)


def margins(info, cam, nviews):
    """Relative distance of the view's estimates from the thresholds that decide for it."""
    e, s = rc.typical_edge_pixels(info.b, cam), rc.depth_spread(info.b, cam)
    out = [abs(e - 5.0) / 5.0, abs(s - 6.0) / 6.0 if np.isfinite(s) else np.inf]
    if nviews == 1 and s <= 6.0:           # (only then does anything ask the spread range)
        out += [abs(e - 10.5) / 10.5, abs(e - 19.0) / 19.0]
    return min(out)


def test_every_estimate_keeps_its_margin():
    """20 % from every threshold: the mean edge counts a grid's diagonals, and a scene near a threshold would test the estimate."""
    for name, (mesh, cam, texels, _, _) in rc.RENDER_CASES.items():
        assert margins(rc.mesh_info(mesh, texels), cam, 1) >= rc.MARGIN, name
    for name, (mesh, cams, texels, _, _, _, _) in rc.GROUP_CASES.items():
        for cam in cams:
            assert margins(rc.mesh_info(mesh, texels), cam, len(cams)) >= rc.MARGIN, name
    # the estimate that is exactly none: the depth of the box centre is 0
    room = rc.RENDER_CASES["room no estimate"]
    assert rc.typical_edge_pixels(rc.mesh_info(room[0]).b, room[1]) == 0.0 and rc.depth_spread(rc.mesh_info(room[0]).b, room[1]) == np.inf


def test_the_restated_dispatch_gives_what_each_case_is_for():
    for name, (mesh, cam, texels, packed, intent) in rc.RENDER_CASES.items():
        e = rc.case_expectation("render", name)
        assert (e["mode"], e["tpw"], e["chunk"], bool(e["stages"] & 2), bool(e["stages"] & 4)) == intent, name
        assert e["fragment_format"] == (8 if e["mode"] & 8 else 10) and bool(e["mode"] & 4) == texels
    for name, (mesh, cams, texels, options, route, intent, minority) in rc.GROUP_CASES.items():
        e = rc.case_expectation("group", name)
        assert (e["kernel"], e["mode"], e["tpw"], bool(e["stages"] & 2)) == intent, name
        assert bool(e["stages"] & 8) == (route == "depth")
        assert e["raster_path"] == ("meshlets" if e["kernel"] == 3 else "vertex-stage")
        assert len({(c.W, c.H) for c in cams}) > 1, name                      # mixed resolutions
        info = rc.mesh_info(mesh, texels)
        assert info.ordered and info.tables
        # the minority views are exactly those whose own verdict the launch overruled
        push, balance = bool(e["mode"] & 1), bool(e["stages"] & 2) or rc.vote([rc.wants_balance(info.b, c) for c in cams])
        overruled = tuple(k for k, c in enumerate(cams) if rc.wants_wg_push(info.b, c) != push or rc.wants_balance(info.b, c) != balance)
        assert overruled == minority, name
    assert sorted(len(rc.GROUP_CASES[n][1]) for n in ("three views", "push vote 2 of 4", "eight views meshlets")) == [3, 4, 8]


def test_votes_ties_and_the_ladder():
    assert [rc.vote(v) for v in ([0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 0], [1, 0, 0], [1], [0])] == [
        False, False, True, True, True, False, True, False]
    g = rc.GROUP_CASES
    for name, votes in (("push vote 1 of 4", 1), ("push vote 2 of 4", 2), ("push vote 3 of 4", 3)):
        mesh, cams = g[name][0], g[name][1]
        assert sum(rc.wants_wg_push(rc.mesh_info(mesh).b, c) for c in cams) == votes and len(cams) == 4
    mesh, cams = g["balance vote 2 of 3"][0], g["balance vote 2 of 3"][1]
    assert [rc.wants_balance(rc.mesh_info(mesh).b, c) for c in cams] == [True, False, True]
    # the ladder: each face count is in the middle of its step, leaves a partial last wave (above one triangle per wave) and a
    # partial last workgroup; block counts on both sides of 64, and with placement on no multiple of 64 (surplus grid blocks)
    for F, (n, tpw, nb) in rc.LADDER.items():
        assert rc.tpw_ladder(F) == tpw and rc.blocks(F, tpw) == nb
        assert (tpw == 1 or F % tpw) and -(-F // tpw) % 4
        assert nb < 64 or nb % 64
    assert min(v[2] for v in rc.LADDER.values()) < 64 < max(v[2] for v in rc.LADDER.values())
    assert 32768 <= 39190 < 65536
    # one view: the steps as the rules say -- and no face count at all stops at 16 triangles per wave
    steps = [(1, 1), (4095, 1), (4096, 2), (8191, 2), (8192, 4), (16383, 4), (16384, 8), (32767, 8), (32768, 32), (65535, 32), (65536, 64)]
    assert [rc.tpw_ladder(F) for F, _ in steps] == [t for _, t in steps]
    assert 16 not in {rc.tpw_ladder(F, n) for F in list(range(1, 70000, 7)) + [32767, 32768] for n in (1, 2, 3, 4, 8)}
    assert rc.tpw_ladder(32768, 2) == 64 and rc.tpw_ladder(32767, 8) == 8
    assert rc.frag_groups(3999999, 8, 64) == 1 and rc.frag_groups(4000000, 8, 64) == 4 and rc.frag_groups(4000000, 1, 64) == 1
    assert rc.frag_groups(4000000, 8, 32) == 1 and [rc.chunk(n) for n in (63, 64)] == [0, 8]
    # every grouped case's block count, both sides of 64 over the table
    nbs = {rc.blocks(rc.mesh_info(m).F, e["tpw"], e["groups"]) for name, (m, *_) in g.items() for e in [rc.case_expectation("group", name)]}
    assert min(nbs) < 64 < max(nbs) and all(n < 64 or n % 64 for n in nbs)


def test_the_decorated_scene_holds_what_it_claims():
    """Boxes by the spec's rule, in numpy: the counts per class, the two runs in single aligned waves, the face order
    kept, and every other triangle of the two waves small."""
    mesh, cam = rc.decorated()
    cls, bw, bh = rc.box_classes(mesh, cam)
    counts = np.bincount(cls, minlength=6)
    assert {k: int(counts[k]) for k in (2, 3, 4, 5)} == rc.DECOR_COUNTS and counts[0] == 0
    assert counts[1] == len(mesh.faces) - sum(rc.DECOR_COUNTS.values())
    run30, run5 = np.arange(rc.RUN_30, rc.RUN_30 + 30), np.arange(rc.RUN_5, rc.RUN_5 + 5)
    assert (cls[run30] == 2).all() and (cls[run5] == 2).all()
    assert len({int(f) // 64 for f in run30}) == 1 and len({int(f) // 64 for f in run5}) == 1 and len({int(f) // 32 for f in run30}) == 1
    for run in (run30, run5):
        wave = np.arange(run[0] // 64 * 64, run[0] // 64 * 64 + 64)
        assert (cls[np.setdiff1d(wave, run)] == 1).all()
    assert 30 >= rc.LANE_BOX_MIN > 5
    lane = cls == 2
    assert (np.maximum(bw, bh)[lane] >= 9).all() and (np.maximum(bw, bh)[lane] <= 24).all() and (bw[lane] * bh[lane] <= 256).all()
    assert (np.maximum(bw, bh)[cls == 3] >= 25).all() and (np.maximum(bw, bh)[cls == 4] > 64).all()
    # no other wave holds a lane-box triangle, and the singles sit in waves of their own
    assert set(np.flatnonzero(lane) // 64) == {rc.RUN_30 // 64, rc.RUN_5 // 64}
    kept, ratio = rc.keeps_face_order(mesh.vertices, mesh.faces)
    assert kept and ratio < 0.8
    info = rc.mesh_info(mesh)
    assert info.tables and abs(rc.typical_edge_pixels(info.b, cam) - rc.DECOR_EDGE) < 0.05


def test_the_other_scenes_hold_their_classes():
    """Sheets at 2.5 and 7 pixels: every box within 8 x 8; at 14: boxes a lane walks; at 30: boxes a wave walks; the room from
    inside: all of them and the near plane.  Every mesh keeps the caller's face order and has meshlet tables."""
    want = {"ladder 66237": {1}, "edge 7 full waves": {0, 1}, "edge 14 spread": {0, 1, 2}, "edge 14 spread few blocks": {2}, "edge 30": {3},
            "room": {0, 1, 2, 3, 4, 5}, "room no estimate": {0, 1, 2, 3, 5}, "room 32 per wave": {0, 1, 2, 5}}
    for name, classes in want.items():
        mesh, cam = rc.RENDER_CASES[name][:2]
        assert set(np.flatnonzero(rc.class_counts(mesh, cam))) == classes, name
    for name, (mesh, cam, texels, _, intent) in rc.RENDER_CASES.items():
        info = rc.mesh_info(mesh, texels)
        assert info.ordered and info.tables, name
        if intent[3]:                                         # a medium stage without a triangle for it has tested nothing
            assert rc.class_counts(mesh, cam)[2:4].sum() > 100, name
    for name, (mesh, cams, *_rest) in rc.GROUP_CASES.items():
        e = rc.case_expectation("group", name)
        if e["stages"] & 2:
            assert sum(rc.class_counts(mesh, c)[2:4].sum() for c in cams) > 100, name


def test_the_report_options_are_read_only():
    """The seven "last_raster_*" options exist without a device, cannot be set, and no other name behind the prefix is one."""
    from semantic_meshes_amd import _lib
    assert _lib.RASTER_REPORT_FIELDS == rc.FIELDS
    report = {f: _lib.get_option("last_raster_" + f) for f in rc.FIELDS}
    assert report["kernel"] in rc.KERNELS and all(v >= 0 for v in report.values())
    if report["kernel"] == 0:                                  # no raster launch on this thread yet
        assert set(report.values()) == {0}
    for f in rc.FIELDS:
        assert _lib.lib().smesh_set_option(("last_raster_" + f).encode(), 1) == _lib.ERR_INVALID
    v = ctypes.c_int64(0)
    assert _lib.lib().smesh_get_option(b"last_raster_", ctypes.byref(v)) == _lib.ERR_INVALID
    assert _lib.lib().smesh_get_option(b"last_raster_modes", ctypes.byref(v)) == _lib.ERR_INVALID
