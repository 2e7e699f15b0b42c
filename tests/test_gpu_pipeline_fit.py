"""The group pipeline's fit of its two kernels into a CU (options "pipeline_fit", "pipeline_fuse_waves", "pipeline_fuse_pad";
common.hpp: pipeline_fuse_pad): the eight-view k_fuse_tri launch over fine views carries an LDS pad -- computed from the device's LDS
and the instance's own, or the constant of before, or none with the pipeline off -- and the pad changes how many workgroups share a CU,
never a result.  The scene is that of tests/test_gpu_fuse_tri_instances.py (the `helpers.small_scene` grid, 6 373 faces: a last block
of 37 rows).
"""
import numpy as np
import pytest

from test_gpu_labels import bits
from test_gpu_fuse_tri_instances import last_fuse, slot, small_inputs, small_triangles

pytestmark = pytest.mark.gpu

OPTIONS = ("group_pipeline", "pipeline_fit", "pipeline_fuse_waves", "pipeline_fuse_pad")
LDS_PER_CU = 163840                     # gfx950
STATIC_LDS = {19: 4880, 17: 6160}       # k_fuse_tri<19, Sum, exact, 8> and the 24-slot run-time-C instance (tools/kernel_regs.sh)


@pytest.fixture
def options(sm):
    """set(name, value); every option this module touches is restored."""
    before = {name: sm._lib.get_option(name) for name in OPTIONS}
    yield sm._lib.set_option
    for name, value in before.items():
        sm._lib.set_option(name, value)


@pytest.mark.parametrize("C", [19, 17], ids=lambda C: "c%02d" % C)
def test_three_calls_with_the_group_pipeline_on_and_off(sm, oracle, options, C):
    """Three consecutive fuse_views calls of sixteen fine views each (two groups of eight: both banks of the renderer, the second
    group's raster beside the first one's fusion) with the group pipeline on -- the eight-view launches carry the computed pad, the
    constant one (option "pipeline_fit" 0), a forced one -- and off (no pad): the raw accumulators are bit-equal to each other and to
    the float32 single-threaded oracle's."""
    from semantic_meshes_amd.device import to_device
    scene = small_triangles(37)
    P = len(scene.faces)
    r = sm.render.triangles(scene)
    probs, weights = small_inputs(C, "sum", scene)
    dp, dw = [to_device(p) for p in probs], [to_device(w) for w in weights]
    order = [k % 8 for k in range(16)]
    oagg = oracle.OracleAggregator(P, C, "sum", 0.5)
    for k in order * 3:
        oagg.add(scene.oidx[k], probs[k], weights[k])
    want_raw = oagg.get_raw()
    pads = {}
    for pipeline, fit, forced in ((1, 1, -1), (1, 0, -1), (1, 1, 1024), (0, 1, -1)):
        options("group_pipeline", pipeline)
        options("pipeline_fit", fit)
        options("pipeline_fuse_pad", forced)
        agg = sm.fusion.MeshAggregator(P, C, "sum", 0.5)
        for _ in range(3):
            agg.fuse_views(r, [scene.cams[k] for k in order], [dp[k] for k in order], [dw[k] for k in order])
            assert last_fuse(sm) == (slot(C), 8)
        pads[(pipeline, fit, forced)] = sm._lib.get_option("last_fuse_lds_pad")
        np.testing.assert_array_equal(bits(agg.get_raw()), bits(want_raw), err_msg="pipeline %d, fit %d, pad %d" % (pipeline, fit, forced))
    assert pads[(0, 1, -1)] == 0 and pads[(1, 0, -1)] == 24576 and pads[(1, 1, 1024)] == 1024
    assert pads[(1, 1, -1)] > 0


@pytest.mark.parametrize("waves", [4, 5, 8])
@pytest.mark.parametrize("C", [19, 17], ids=lambda C: "c%02d" % C)
def test_the_computed_pad_caps_the_launch_at_the_wanted_waves(sm, options, C, waves):
    """`waves` workgroups of static + pad bytes fit a CU's LDS and one more does not, whatever allocation granule (a divisor of 1 280
    bytes) the hardware rounds a workgroup up to; and the pad leaves the meshlet rasteriser of this renderer at least one workgroup."""
    from semantic_meshes_amd.device import to_device
    scene = small_triangles(37)
    P = len(scene.faces)
    r = sm.render.triangles(scene)
    probs, weights = small_inputs(C, "sum", scene)
    options("group_pipeline", 1)
    options("pipeline_fit", 1)
    options("pipeline_fuse_pad", -1)
    options("pipeline_fuse_waves", waves)
    agg = sm.fusion.MeshAggregator(P, C, "sum", 0.5)
    agg.fuse_views(r, scene.cams, [to_device(p) for p in probs], [to_device(w) for w in weights])
    assert last_fuse(sm) == (slot(C), 8)
    wg = STATIC_LDS[C] + sm._lib.get_option("last_fuse_lds_pad")
    for granule in (128, 256, 640, 1280):
        rounded = -(-wg // granule) * granule
        assert waves * rounded <= LDS_PER_CU < (waves + 1) * rounded, (wg, granule)
    assert wg <= 65536
    assert sm._lib.get_option("last_fuse_beside") >= 1
