"""Every compiled instance of the rasteriser (semantic_meshes_amd/csrc/raster.hip), launched where the library itself picks it and
compared with the CPU oracle.

The host picks one of about 35 compiled kernels per launch -- k_raster_frag<MODE> / k_raster_frag_group<MODE> for nine modes,
k_raster_frag_group_ml<MODE> for three, the medium, huge and resolve stages -- from estimates of the view (typical edge, depth
spread), the mesh's size and three options.  tests/raster_instances_cases.py restates that dispatch once, in numpy, and builds the
smallest scenes on either side of each rule; tests/test_raster_instances_host.py checks the restatement and the scenes without a GPU.
Here every case is launched, and the launch's own report (the read-only options "last_raster_kernel" / "_mode" / "_views" / "_tpw" /
"_groups" / "_chunk" / "_stages", plus last_raster_path, "last_record_format" and "last_fragment_format") must be what the
restatement says.

(a) render(): index plane and depth bits equal to the oracle's; the queue lengths of smesh_renderer_render_stats non-zero exactly for
    the box classes the scene holds by the spec's box rule (exactly those counts where no triangle crosses the near plane unseen).
(b) fuse_views of 3, 4 and 8 views of mixed resolutions (C = 19, Sum, random class vectors on the device): the raw accumulator
    bit-equal to the float32 single-threaded oracle where every box stays within 8 x 8 pixels, else get() against the
    float64-accumulating oracle at rtol 1e-5, atol 1e-6.  The views a vote overruled (they run in the majority's instance) are also
    fused with the other views' class vectors zeroed -- their contribution alone, within the group's launch -- and alone.
(c) what only a test hook reaches (raster_instances_cases.HOOKS: spread waves in a grouped launch, a medium stage behind spread waves,
    four groups of 64 triangles per wave): the same cases in one fresh child process per knob setting, the same assertions.

Durations on an MI355X (DURATIONS below): the whole module, 48 tests, 12.9 s, 3.4 s of it the first use of the device; of that the
children of part (c) 2.33 (spread), 1.79 (spread-balance) and 4.55 s (groups), the largest of two runs each, interpreter and library
start-up included; an in-process case at most 0.16 s.
"""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import edge_gate_ref as eg
import raster_instances_cases as rc
from helpers import assert_fused_close, random_probs
from test_gpu_labels import bits

pytestmark = pytest.mark.gpu

# Measured on an MI355X (seconds): the children of part (c), the whole module and its slowest in-process case.  A child's timeout is
# three times its duration, rounded up to 10 s.
DURATIONS = {"spread": 2.33, "spread-balance": 1.79, "groups": 4.55, "module": 12.9, "slowest": 0.16}
CHILD_TIMEOUT = {key: int(-(-3 * d // 10) * 10) for key, d in DURATIONS.items() if key not in ("module", "slowest")}

CHILD = os.environ.get("SMESH_RASTER_INSTANCES_CHILD", "")           # the knob setting this process runs under (part (c)), or ""
KNOBS = rc.HOOKS[CHILD.replace("-", " ")][1] if CHILD else rc.NO_KNOBS
GATE = (3, 0.15, 0.01, True, True, True)
TEXELS_PER_PIXEL = 1.0
OBSERVED = set()                                 # instance names seen through the launches' reports in this process
RAN = set()                                      # (kind, case) that ran in this process


@contextlib.contextmanager
def options(sm, **values):
    """Set options in-process through smesh_set_option; the values found are restored."""
    before = {k: sm._lib.get_option(k) for k in values}
    try:
        for k, v in values.items():
            sm._lib.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            sm._lib.set_option(k, v)


def camera(sm, cam):
    return sm.data.Camera(cam.R, cam.t, np.asarray([cam.W, cam.H]), np.asarray([cam.fx, cam.fy], np.float64), np.asarray([cam.cx, cam.cy], np.float64))


def texel_cameras(mesh, cams):
    """The cameras a texel renderer sizes its texels by: the case's own -- the room's: the view from outside (from inside, a triangle at
    the camera plane would ask for millions of texels)."""
    return [rc.outside()] if mesh is rc.room(24) else list(cams)


def renderers(sm, oracle, mesh, texels, cams):
    """(the library's renderer, the oracle's) of a case."""
    if not texels:
        return sm.render.triangles(sm.data.Mesh(mesh.vertices, mesh.faces)), oracle.OracleRenderer(mesh.vertices, mesh.faces)
    tc = [camera(sm, c) for c in texel_cameras(mesh, cams)]
    r = sm.render.texels(sm.data.Mesh(mesh.vertices, mesh.faces), tc, TEXELS_PER_PIXEL)
    o = oracle.OracleRenderer(mesh.vertices, mesh.faces, tc, TEXELS_PER_PIXEL)
    assert r.getPrimitivesNum() == o.getPrimitivesNum() >= len(mesh.faces)
    return r, o


def assert_report(sm, want, what):
    """All seven reported values and the two formats against the restated dispatch; returns the report."""
    got = sm._lib.last_raster_instance()
    assert got == {f: want[f] for f in rc.FIELDS}, (what, got, want)
    assert sm._lib.get_option("last_record_format") == want["record_format"], what
    assert sm._lib.get_option("last_fragment_format") == want["fragment_format"], what
    OBSERVED.update(rc.instances_of(got))
    return got


def assert_queues(r, cam, mesh, c, want, what):
    """The queue lengths the launch left against the scene's box classes (raster_instances_cases.box_classes)."""
    needed, q = r.render_stats(cam, queues=True)
    counts = rc.class_counts(mesh, c)
    print("    %s: box classes %s, queues %s" % (what, list(counts), q))
    assert needed == bool(want["stages"] & 4), what
    assert q[1] == 0, what                                              # no queue overflowed
    cls, bw, bh = rc.box_classes(mesh, c)
    over, huge, crossing = int(counts[2:5].sum()), int(counts[4]), int(counts[5])
    mid = int(((cls >= 2) & (cls <= 4) & (bw * bh <= 256)).sum())         # entries of at most 256 box pixels
    if mesh is rc.decorated()[0] or not crossing:                       # (the decorated scene's crossing triangles all reach the image)
        assert (q[0], q[2]) == (over + crossing, huge + crossing), what
    else:                                                               # the room: a crossing triangle's front piece may miss the image
        assert 0 < over <= q[0] <= over + crossing and huge <= q[2] <= huge + crossing, what
        assert q[0] - over == q[2] - huge, what                         # (whichever of them did reach it is in both queues)
    assert mid <= q[3] <= mid + crossing, what


# ---- (a) render() ---------------------------------------------------------------------------------------------------------------------
def run_render_case(sm, oracle, name):
    mesh, c, texels, packed, _ = rc.RENDER_CASES[name]
    want = rc.case_expectation("render", name, KNOBS)
    with options(sm, packed_fragments=packed):
        r, o = renderers(sm, oracle, mesh, texels, [c])
        cam = camera(sm, c)
        path = sm._lib.last_raster_path()
        idx, depth = r.render(cam, lazy=False)                          # (the Python layer defers render(): this launches now)
        assert_report(sm, want, name)
        assert sm._lib.last_raster_path() == path                      # (a grouped launch's report: untouched)
        assert_queues(r, cam, mesh, c, want, name)
        oidx, odepth = o.render(cam)
        assert (oidx != 0xFFFFFFFF).mean() > 0.3, name
        np.testing.assert_array_equal(np.asarray(idx), oidx, err_msg=name)
        np.testing.assert_array_equal(np.asarray(depth).view(np.uint32), odepth.view(np.uint32), err_msg=name)
    RAN.add(("render", name))


@pytest.mark.parametrize("name", list(rc.RENDER_CASES), ids=lambda n: n.replace(" ", "-"))
def test_render_picks_the_instance_and_equals_the_oracle(sm, oracle, name):
    """Part (a): one render() per case of RENDER_CASES."""
    run_render_case(sm, oracle, name)


# ---- (b) grouped launches -------------------------------------------------------------------------------------------------------------
def fused(sm, r, P, cams, dev, route):
    agg = sm.fusion.MeshAggregator(P, rc.C)
    if route == "depth":
        agg.fuse_views(r, cams, dev, edge_gate=sm.fusion.EdgeGate(*GATE))
    else:
        agg.fuse_views(r, cams, dev)
    return agg


def oracle_fused(oracle, P, oidx, probs, weights, double):
    oracle.set_accum_double(double)
    try:
        oagg = oracle.OracleAggregator(P, rc.C)
        for k in range(len(oidx)):
            oagg.add(oidx[k], probs[k], None if weights is None else weights[k])
        return oagg.get_raw(), oagg.get()
    finally:
        oracle.set_accum_double(False)


def compare(agg, oracle, P, oidx, probs, weights, small, what):
    if small:
        raw, dist = oracle_fused(oracle, P, oidx, probs, weights, False)
        assert np.abs(raw).sum() > 0, what
        np.testing.assert_array_equal(bits(agg.get_raw()), bits(raw), err_msg=what)
        np.testing.assert_array_equal(bits(agg.get()), bits(dist), err_msg=what)
    else:
        _, dist = oracle_fused(oracle, P, oidx, probs, weights, True)
        assert (dist.sum(axis=1) > 0.5).sum() > 100, what
        assert_fused_close(agg.get(), dist, rtol=1e-5, atol=1e-6)


def run_group_case(sm, oracle, name):
    from semantic_meshes_amd.device import to_device
    mesh, cs, texels, opts, route, _, minority = rc.GROUP_CASES[name]
    want = rc.case_expectation("group", name, KNOBS)
    small = all(rc.class_counts(mesh, c)[2:].sum() == 0 for c in cs)
    with options(sm, **opts):
        r, o = renderers(sm, oracle, mesh, texels, cs)
        P, cams = r.getPrimitivesNum(), [camera(sm, c) for c in cs]
        rng = np.random.default_rng(len(name))
        probs = [random_probs(rng, c.W, c.H, rc.C) for c in cs]
        dev = [to_device(p) for p in probs]
        rendered = [o.render(cam) for cam in cams]
        oidx = [i for i, _ in rendered]
        weights = [eg.weights(d, eg.gate(*GATE))[0] for _, d in rendered] if route == "depth" else None
        agg = fused(sm, r, P, cams, dev, route)
        assert_report(sm, want, name)
        assert sm._lib.last_raster_path() == want["raster_path"], name
        compare(agg, oracle, P, oidx, probs, weights, small, name)
        for k in minority:
            # the overruled view's contribution alone: inside the group's launch (the other views' class vectors zero) ...
            alone = [p if j == k else np.zeros_like(p) for j, p in enumerate(probs)]
            agg = fused(sm, r, P, cams, [d if j == k else to_device(alone[j]) for j, d in enumerate(dev)], route)
            assert_report(sm, want, "%s, view %d within the group" % (name, k))
            compare(agg, oracle, P, oidx, alone, weights, small, "%s, view %d within the group" % (name, k))
            # ... and by itself, in the instance of its own verdict
            agg = sm.fusion.MeshAggregator(P, rc.C)
            agg.fuse_view(r, cams[k], dev[k])
            got = sm._lib.last_raster_instance()
            own = rc.expected_render(rc.mesh_info(mesh, texels), cs[k], bool(opts.get("packed_fragments", 1)), False, KNOBS)
            assert {f: got[f] for f in ("kernel", "mode", "tpw", "chunk")} == {f: own[f] for f in ("kernel", "mode", "tpw", "chunk")}, (name, k, got)
            if not CHILD:
                assert (got["mode"] & 1, bool(got["stages"] & 2)) != (want["mode"] & 1, bool(want["stages"] & 2)), (name, k)
            OBSERVED.update(rc.instances_of(got))
            compare(agg, oracle, P, oidx[k:k + 1], probs[k:k + 1], None if weights is None else weights[k:k + 1],
                    rc.class_counts(mesh, cs[k])[2:].sum() == 0, "%s, view %d alone" % (name, k))
    RAN.add(("group", name))


@pytest.mark.parametrize("name", list(rc.GROUP_CASES), ids=lambda n: n.replace(" ", "-"))
def test_fuse_views_picks_the_instance_and_equals_the_oracle(sm, oracle, name):
    """Part (b): one fuse_views call per case of GROUP_CASES, and the overruled views of the vote cases by themselves."""
    run_group_case(sm, oracle, name)


def test_every_instance_was_observed():
    """At module end: when all of parts (a) and (b) ran in this process, every instance the library can pick by itself was launched
    and asserted by name, and none of the hook-only ones."""
    if CHILD or not RAN >= {("render", n) for n in rc.RENDER_CASES} | {("group", n) for n in rc.GROUP_CASES}:
        return
    assert rc.LIBRARY_INSTANCES <= OBSERVED, sorted(rc.LIBRARY_INSTANCES - OBSERVED)
    assert not OBSERVED & rc.HOOK_ONLY


# ---- (c) what only a hook reaches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [k.replace(" ", "-") for k in rc.HOOKS])
def test_hook_only_instances_in_child_processes(sm, oracle, knob):
    """The knobs are read once per process: the cases of HOOKS[knob] in a fresh child process under the knob's environment, with the
    assertions of parts (a) and (b) against the dispatch restated WITH the knob -- and the instances and launch shapes the knob is for
    among what the launches reported."""
    env, knobs, cases = rc.HOOKS[knob.replace("-", " ")]
    if CHILD != knob:
        t0 = time.time()
        res = subprocess.run([sys.executable, "-m", "pytest", "%s::test_hook_only_instances_in_child_processes[%s]" % (os.path.abspath(__file__), knob),
                              "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider"],
                             env=dict(os.environ, SMESH_RASTER_INSTANCES_CHILD=knob, **env), capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT[knob])
        print("    child %s: %.2f s" % (knob, time.time() - t0))
        assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
        assert "hook-only ok: %s" % knob in res.stdout, res.stdout[-1000:]
        return
    shapes = set()
    for kind, name in cases:
        (run_render_case if kind == "render" else run_group_case)(sm, oracle, name)
        got = sm._lib.last_raster_instance() if kind == "render" else rc.case_expectation(kind, name, knobs)
        shapes.add((got["kernel"], bool(got["mode"] & 2), bool(got["stages"] & 2), got["groups"]))
    assert rc.HOOK_INSTANCES.get(CHILD.replace("-", " "), set()) <= OBSERVED, sorted(OBSERVED)
    if knob == "spread-balance":
        assert {(1, True, True, 1), (2, True, True, 1)} <= shapes
    if knob == "groups":
        assert {s[3] for s in shapes} == {4}
    print("hook-only ok: %s %s" % (knob, sorted(OBSERVED)))
