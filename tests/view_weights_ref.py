"""numpy restatement of include/smesh_view_weights.h: the face normals, the viewing-geometry weights of one view and their counts, every
step a single IEEE operation in the header's order (float32, the ray's a and b in float64 rounded once), and the floor scene of the
tests.  Shared by test_view_weights_host.py and test_gpu_view_weights.py; nothing here calls the product's library (cameras are
semantic_meshes_amd.data.Camera objects, which are plain Python)."""
import collections
import math

import numpy as np

# power: int 0 .. 16; min_cos, max_depth, falloff_depth: float32 values (+inf: none); two_sided: bool
Spec = collections.namedtuple("Spec", "power min_cos two_sided max_depth falloff_depth")

VISIBLE, FAR, GRAZING, BACKFACING = 0, 1, 2, 3
BG = np.uint32(0xFFFFFFFF)
MAX_POWER = 16


def spec(power=1, min_cos=0.0, two_sided=True, max_depth=None, falloff_depth=None):
    """The spec of `fusion.ViewWeights(power, min_cos, two_sided, max_depth, falloff_depth)`: the defaults of the Python layer, every
    number rounded to float32 once."""
    assert 0 <= int(power) <= MAX_POWER
    inf = np.float32(np.inf)
    return Spec(int(power), np.float32(min_cos), bool(two_sided), inf if max_depth is None else np.float32(max_depth),
                inf if falloff_depth is None else np.float32(falloff_depth))


def face_normals(vertices, faces):
    """float32 [F,3]: n = (v1 - v0) x (v2 - v0), each component two multiplies and one subtract; not normalised; (0, 0, 0) for a face
    with a vertex index outside [0, V)."""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert n.dtype == np.float32
    n[~ok] = 0.0
    return n


def rays(cam):
    """(a float32 [W], b float32 [H]): ((X + 0.5) - cx) / fx and ((Y + 0.5) - cy) / fy in float64, each rounded to float32."""
    W, H = cam.resolution
    fx, fy = (np.float64(v) for v in cam.focal_lengths)
    cx, cy = (np.float64(v) for v in cam.principal_point)
    a = (((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx).astype(np.float32)
    b = (((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy).astype(np.float32)
    return a, b


def cosines(cam, normals, idx, depth):
    """(c, dot, visible) of the header's steps 1 and 3 for every pixel: float32 (W,H) cosine (0 for a degenerate face and for
    background), float32 dot, and the mask of the pixels that pass step 1."""
    idx, d_r = np.asarray(idx), np.asarray(depth)
    assert idx.dtype == np.uint32 and d_r.dtype == np.float32 and idx.shape == d_r.shape == tuple(cam.resolution)
    n = np.asarray(normals, np.float32)
    F = len(n)
    visible = np.isfinite(d_r) & (idx != BG) & (idx.astype(np.int64) < F)
    nf = n[np.where(visible, idx, 0).astype(np.int64)] if F else np.zeros(idx.shape + (3,), np.float32)
    R = np.asarray(cam.rotation, np.float32)
    a, b = rays(cam)
    a, b = a[:, None], b[None, :]
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        nc = [(R[r, 0] * nf[..., 0] + R[r, 1] * nf[..., 1]) + R[r, 2] * nf[..., 2] for r in range(3)]
        dot = (nc[0] * a + nc[1] * b) + nc[2]
        nn = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
        dd = (a * a + b * b) + one
        nd = nn * dd
        ok = (nn > 0) & np.isfinite(nd)
        c = np.where(ok, np.abs(dot) / np.sqrt(np.where(ok, nd, one)), np.float32(0.0))
    assert dot.dtype == nn.dtype == nd.dtype == c.dtype == np.float32
    return c, dot, visible


def weights(cam, normals, idx, depth, s, weights_in=None):
    """(float32 (W,H) weights, uint64 [visible, far, grazing, backfacing]) of one view: `idx` uint32 (W,H) with 0xFFFFFFFF for
    background, `depth` float32 (W,H) with +inf for background, `normals` float32 [F,3] by face id, `s` a Spec, `weights_in` float32
    (W,H) or None (all ones)."""
    d_r = np.asarray(depth)
    W, H = d_r.shape
    w_in = np.ones((W, H), np.float32) if weights_in is None else np.asarray(weights_in)
    assert w_in.dtype == np.float32 and w_in.shape == (W, H)
    c, dot, visible = cosines(cam, normals, idx, depth)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        far = visible & (d_r > s.max_depth)
        back = visible & ~far & (dot > 0) if not s.two_sided else np.zeros((W, H), bool)
        grazing = visible & ~far & ~back & ~(c >= s.min_cos)
        g = np.ones((W, H), np.float32)
        for _ in range(s.power):
            g = g * c
        f = np.ones((W, H), np.float32)
        if np.isfinite(s.falloff_depth):
            q = np.where(visible, d_r, one) / s.falloff_depth
            f = one / (one + q * q)
        w = (w_in * g) * f
    assert g.dtype == f.dtype == w.dtype == np.float32
    out = np.where(visible & ~far & ~back & ~grazing, w, np.float32(0.0)).astype(np.float32)
    counts = np.array([visible.sum(), far.sum(), grazing.sum(), back.sum()], np.uint64)
    return out, counts


# ---- the tilted quad (host test) and the floor scene (effect test) -----------------------------------------------------------------
def quad_mesh(half=4.0):
    """(vertices, faces) of one planar quad z = 0 over [-half, half]^2, two triangles, normal +z."""
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def tilted_camera(tilt_degrees, W, H, distance=6.0, focal=None):
    """A camera that looks at the origin from `distance` away, its axis tilted by `tilt_degrees` from the quad's normal (+z), in the
    x-z plane."""
    from semantic_meshes_amd import synth
    from semantic_meshes_amd.data import Camera
    t = math.radians(tilt_degrees)
    eye = (distance * math.sin(t), 0.0, distance * math.cos(t))
    R, tr = synth.look_at(eye, (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    f = 0.8 * W if focal is None else focal
    return Camera(R, tr, np.asarray([W, H]), np.asarray([f, f], np.float64), np.asarray([W / 2.0, H / 2.0], np.float64))


def plane_render(cam, z=0.0, half=4.0):
    """The index and depth planes a renderer would give for quad_mesh() seen by `cam`, computed analytically in float64 (ray / plane
    intersection; face 0 below the diagonal x > y ... the split does not matter to the tests: both faces share the normal)."""
    W, H = cam.resolution
    R = np.asarray(cam.rotation, np.float64)
    t = np.asarray(cam.translation, np.float64)
    eye = -R.T @ t
    fx, fy = cam.focal_lengths
    cx, cy = cam.principal_point
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="ij")
    d_cam = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], axis=-1)
    d_world = d_cam @ R                                   # R^T d, row form
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (z - eye[2]) / d_world[..., 2]                # depth along the camera's axis, since d_cam's z is 1
    p = eye + s[..., None] * d_world
    hit = np.isfinite(s) & (s > 1e-6) & (np.abs(p[..., 0]) < half) & (np.abs(p[..., 1]) < half)
    idx = np.where(hit, np.where(p[..., 0] - p[..., 1] > 0, 0, 1), 0xFFFFFFFF).astype(np.uint32)
    depth = np.where(hit, s, np.inf).astype(np.float32)
    return idx, depth, d_world
