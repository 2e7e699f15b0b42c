"""numpy restatement of include/smesh_depth.h: the depth-consistency weights of one view and their counts, every step a single float32
operation in the header's order, and the occluder scene of the tests.  Shared by test_depth_gate_host.py and test_gpu_depth_gate.py;
nothing here calls the product's library (the scene takes its mesh and cameras from semantic_meshes_amd.synth, which is numpy)."""
import collections

import numpy as np

# scale, abs_tol, rel_tol: float32 values; max_depth: float32, +inf for none; missing_keep: bool
Gate = collections.namedtuple("Gate", "scale abs_tol rel_tol max_depth missing_keep")

VISIBLE, FAR, MISSING, INCONSISTENT = 0, 1, 2, 3


def gate(abs_tol, rel_tol=0.0, scale=None, max_depth=None, missing="keep", dtype=np.uint16):
    """The gate of `fusion.DepthGate(abs_tol, rel_tol, scale, max_depth, missing)` for a sensor image of `dtype`: the defaults of
    the Python layer, every number rounded to float32 once."""
    if scale is None:
        scale = 0.001 if np.dtype(dtype).kind in "iu" else 1.0
    return Gate(np.float32(scale), np.float32(abs_tol), np.float32(rel_tol), np.float32(np.inf if max_depth is None else max_depth), missing == "keep")


def axis_index(n, N):
    """x = ((2X + 1) n) div (2N) for X in [0, N): nearest neighbour with half-pixel centres, in integers."""
    X = np.arange(N, dtype=np.int64)
    return ((2 * X + 1) * n) // (2 * N)


def sample(sensor, W, H):
    """(w,h) -> (W,H), the sensor's own dtype."""
    sensor = np.asarray(sensor)
    w, h = sensor.shape
    return sensor[axis_index(w, W)[:, None], axis_index(h, H)[None, :]]


def missing_samples(raw):
    """A uint16 sample is missing when it is 0, a float32 sample when !(raw > 0) or it is not finite."""
    if raw.dtype == np.uint16:
        return raw == 0
    assert raw.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return ~(raw > 0) | ~np.isfinite(raw)


def weights(depth, sensor, g, weights_in=None):
    """(float32 (W,H) weights, uint64 [visible, far, missing, inconsistent]) of one view: `depth` float32 (W,H) with +inf for
    background, `sensor` (w,h) uint16 or float32, `g` a Gate, `weights_in` float32 (W,H) or None (all ones)."""
    d_r = np.asarray(depth)
    assert d_r.dtype == np.float32 and d_r.ndim == 2
    W, H = d_r.shape
    raw = sample(sensor, W, H)
    w_in = np.ones((W, H), np.float32) if weights_in is None else np.asarray(weights_in)
    assert w_in.dtype == np.float32 and w_in.shape == (W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        d_s = raw.astype(np.float32) * g.scale
        t = g.abs_tol + g.rel_tol * d_s            # a multiply, then an add
        diff = np.abs(d_r - d_s)
        assert d_s.dtype == t.dtype == diff.dtype == np.float32
        visible = np.isfinite(d_r)
        far = visible & (d_r > g.max_depth)
        miss = visible & ~far & missing_samples(raw)
        bad = visible & ~far & ~miss & ~(diff <= t)
    out = np.where(visible & ~far & ~bad & (~miss | g.missing_keep), w_in, np.float32(0.0)).astype(np.float32)
    counts = np.array([visible.sum(), far.sum(), miss.sum(), bad.sum()], np.uint64)
    return out, counts


# ---- the occluder scene --------------------------------------------------------------------------------------------------------
OCCLUDER_SIZES = ((160, 120), (96, 64))
OCCLUDER_VIEWS = 9
_scenes = {}


def occluder_scene(oracle, W, H):
    """(mesh, cameras, oracle index planes, oracle depth planes, sensor images, masks of the pixels the quad covers): the fused mesh is synth.grid_mesh(40, 20); the sensor
    of each of the nine ring cameras saw that mesh PLUS one quad at z = 1.5 over x in [-2, 2], y in [-1.5, 1.5], which is not in the
    fused mesh -- the oracle's render of both, as uint16 millimetres (rint(1000 d), 0 for background).  Built once per size and left
    unchanged."""
    if (W, H) not in _scenes:
        from semantic_meshes_amd import synth
        mesh = synth.grid_mesh(40, 20)
        cams = [synth.ring_camera(k, OCCLUDER_VIEWS, W, H) for k in range(OCCLUDER_VIEWS)]
        V = len(mesh.vertices)
        quad = np.array([[-2, -1.5, 1.5], [2, -1.5, 1.5], [2, 1.5, 1.5], [-2, 1.5, 1.5]], np.float32)
        verts = np.concatenate([np.asarray(mesh.vertices, np.float32), quad])
        faces = np.concatenate([np.asarray(mesh.faces, np.int32), np.array([[V, V + 1, V + 2], [V, V + 2, V + 3]], np.int32)])
        o_mesh, o_seen = oracle.OracleRenderer(mesh.vertices, mesh.faces), oracle.OracleRenderer(verts, faces)
        oidx, odepth, sensors, covered = [], [], [], []
        for cam in cams:
            idx, depth = o_mesh.render(cam)
            sidx, sdepth = o_seen.render(cam)
            with np.errstate(invalid="ignore"):
                mm = np.where(np.isfinite(sdepth), np.rint(np.float64(1000.0) * sdepth), 0.0)
            assert mm.max() < 65535
            oidx.append(idx)
            odepth.append(depth)
            sensors.append(mm.astype(np.uint16))
            covered.append((sidx >= len(mesh.faces)) & (sidx != np.uint32(0xFFFFFFFF)))
        _scenes[(W, H)] = (mesh, cams, oidx, odepth, sensors, covered)
    return _scenes[(W, H)]
