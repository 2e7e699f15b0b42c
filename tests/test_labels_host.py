"""Label-image fusion (include/smesh_labels.h, MeshAggregator.add_labels), the part that needs no GPU: the extension header and its
ctypes table, the host-side narrowing rule, the numpy model of the semantics against the CPU oracle, and the source tree's hygiene."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "smesh_labels.h")
HEADER = os.path.join(ROOT, "include", "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")

LABEL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def one_hot(labels, C):
    """tf.one_hot: float32 (..., C); a label outside [0, C), negative values included, is the all-zero vector."""
    labels = np.asarray(labels)
    out = np.zeros(labels.shape + (C,), np.float32)
    wide = labels.astype(np.int64) if labels.dtype != np.uint64 else np.where(labels < C, labels, C).astype(np.int64)
    ok = (wide >= 0) & (wide < C)
    idx = np.nonzero(ok)
    out[idx + (wide[ok],)] = 1.0
    return out


def test_extension_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", EXT_HEADER])
    from semantic_meshes_amd import _lib
    ext = _declared(EXT_HEADER)
    assert ext == sorted(["smesh_fuse_view_labels", "smesh_fuse_views_labels", "smesh_aggregator_add_labels"])
    assert sorted(_lib.EXT_SIGNATURES) == ext
    assert sorted(_lib.SIGNATURES) == _declared(HEADER)            # the pinned ABI is what it was
    assert not set(ext) & set(_declared(HEADER))
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in ext:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    codes = dict(re.findall(r"#define\s+SMESH_LBL_([A-Z0-9]+)\s+(\d+)", open(EXT_HEADER).read()))
    assert {("uint" if k[0] == "U" else "int") + k[1:]: int(v) for k, v in codes.items()} == _lib.LBL_CODES


@pytest.mark.parametrize("C", [2, 19, 255, 256, 1000])
@pytest.mark.parametrize("dtype", LABEL_DTYPES)
def test_narrow_labels_keeps_the_one_hot(dtype, C):
    from semantic_meshes_amd.fusion import narrow_labels
    rng = np.random.default_rng(C * 31 + np.dtype(dtype).num)
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -3), min(info.max, C + 3)
    labels = rng.integers(lo, hi, size=(37, 23), endpoint=True).astype(dtype)
    labels[0, :4] = [info.min, info.max, 0, min(C - 1, info.max)]
    plane = narrow_labels(labels, C)
    assert plane.dtype == (np.uint8 if C <= 255 else np.uint16)
    assert plane.shape == labels.shape and plane.flags.c_contiguous
    code = np.iinfo(plane.dtype).max
    assert code >= C                                               # the don't-care code is never a class
    got = one_hot(np.where(plane == code, -1, plane.astype(np.int64)), C)
    np.testing.assert_array_equal(got, one_hot(labels, C))
    # a strided view (a mask decoded as (H,W), seen as (W,H)) narrows to the same plane
    np.testing.assert_array_equal(narrow_labels(np.ascontiguousarray(labels.T).T, C), plane)


def test_narrow_labels_refuses_floats():
    from semantic_meshes_amd.fusion import narrow_labels
    with pytest.raises(ValueError):
        narrow_labels(np.zeros((4, 4), np.float32), 5)


def labels_model(P, C, iew, views):
    """The semantics section of the label entry points as a float32 numpy loop: views = [(idx (W,H) uint32, labels (W,H) int, weights
    (W,H) float32 or None)]; pixels in image order (x major, y fastest), view after view."""
    acc = np.zeros((P, C), np.float32)
    iew = np.float32(iew)
    one = np.float32(1.0)
    for idx, labels, weights in views:
        n = np.bincount(idx[idx < P].ravel(), minlength=P)
        W, H = idx.shape
        for x in range(W):
            for y in range(H):
                p, c = int(idx[x, y]), int(labels[x, y])
                if p >= P or not 0 <= c < C:
                    continue
                w0 = np.float32(iew * (one / np.float32(n[p]))) + np.float32((one - iew) * one)
                w = np.float32(w0 * (weights[x, y] if weights is not None else one))
                acc[p, c] = np.float32(acc[p, c] + np.float32(one * w))
    return acc


@pytest.mark.parametrize("kind", ["sum", "summax"])
@pytest.mark.parametrize("iew", [0.0, 0.3, 0.5, 1.0])
def test_numpy_model_of_the_label_semantics_is_bit_equal_to_the_oracle_on_one_hot(oracle, kind, iew):
    rng = np.random.default_rng(int(iew * 10) + (100 if kind == "sum" else 200))
    P, C, W, H = 60, 7, 24, 18
    for with_weights in (False, True):
        views = []
        o = oracle.OracleAggregator(P, C, kind, iew)
        for _ in range(4):
            idx = rng.integers(0, P + 6, size=(W, H)).astype(np.uint32)
            idx[idx >= P] = 0xFFFFFFFF
            labels = rng.integers(-2, C + 2, size=(W, H), endpoint=True).astype(np.int32)
            weights = rng.uniform(0.1, 2.0, size=(W, H)).astype(np.float32) if with_weights else None
            views.append((idx, labels, weights))
            o.add(idx, one_hot(labels, C), weights)
        np.testing.assert_array_equal(labels_model(P, C, iew, views).view(np.uint32), o.get_raw().view(np.uint32))


FORBIDDEN = ["s_" + "store_dword", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic_", "s_buffer_" + "atomic", "s_dcache_" + "wb",
             "s_dcache_" + "discard"]


def test_source_tree_holds_no_scalar_stores_and_no_fuse_tri_instance_file_changed():
    for top in ["semantic_meshes_amd", "semantic_meshes", "include", "tools", "tests", "oracle", "."]:
        for base, dirs, files in os.walk(os.path.join(ROOT, top)):
            if top == ".":
                dirs[:] = []
            dirs[:] = [d for d in dirs if d not in ("__pycache__", "_ref", "_san", "golden", ".git")]
            for name in files:
                if name.endswith((".md", ".rst", ".txt", ".json", ".csv", ".so", ".o", ".pyc", ".a", ".ply", ".npy", ".npz", ".png")):
                    continue
                blob = open(os.path.join(base, name), "rb").read().lower()
                for word in FORBIDDEN:
                    assert word.encode() not in blob, "%s holds %s" % (os.path.join(base, name), word)
    # the label kernels live in a translation unit of their own: the files that define and instantiate k_fuse_tri's several-view
    # instances, and the kernel's text, do not know about them
    for rel in ["fuse_tri.inc.hpp", "fuse_mid.inc.hpp", "fusion_pair.hip", "fusion_multi4.hip", "fusion_multi8.hip"]:
        text = open(os.path.join(ROOT, "semantic_meshes_amd", "csrc", rel)).read()
        assert "label" not in text.lower(), rel
