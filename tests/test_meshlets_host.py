"""The meshlet tables of the grouped rasteriser (include/smesh_meshlets.h), the part that needs no GPU: the host builder through its
C entry point, its extension header and ctypes table, and the same builder under AddressSanitizer / UBSan in a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smesh_meshlets.h")
CSRC = os.path.join(ROOT, "semantic_meshes_amd", "csrc")
TRIS, CAP, BITS = 256, 384, 10


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def build(faces, V):
    """(has_meshlets, first, ids, tris) of int32 faces [F, 3] through smesh_meshlets_build."""
    from semantic_meshes_amd import _lib
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = len(faces)
    blocks = (F + TRIS - 1) // TRIS
    first = np.full(blocks + 1, 0xDEADBEEF, np.uint32)
    ids = np.full(max(3 * F, 1), 0xDEADBEEF, np.uint32)
    tris = np.full(max(F, 1), 0xDEADBEEF, np.uint32)
    used, has = ctypes.c_uint64(0), ctypes.c_int(-1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(_lib.lib().smesh_meshlets_build(p(faces), F, V, p(first), p(ids), len(ids), p(tris), ctypes.byref(used), ctypes.byref(has)))
    assert has.value in (0, 1)
    return bool(has.value), first, ids[:used.value], tris[:F]


def grid(a, b, keep=None):
    from semantic_meshes_amd import synth
    m = synth.grid_mesh(a, b)
    return np.asarray(m.faces, np.int32)[:keep], len(m.vertices)


def check_tables(faces, V, first, ids, tris):
    F = len(faces)
    blocks = (F + TRIS - 1) // TRIS
    assert first[0] == 0 and first[blocks] == len(ids) and (np.diff(first.astype(np.int64)) >= 0).all()
    counts = np.diff(first.astype(np.int64))
    assert counts.max(initial=0) <= CAP                                           # the counts stay within the cap
    block = np.arange(F) // TRIS
    local = np.stack([(tris >> (BITS * k)) & ((1 << BITS) - 1) for k in range(3)], axis=1).astype(np.int64)
    assert (local < counts[block][:, None]).all()                                  # every local index is below its block's count
    decoded = ids[first[block].astype(np.int64)[:, None] + local]
    assert np.array_equal(decoded.astype(np.int64), faces.astype(np.int64))        # decoding reproduces `faces` exactly
    assert (ids < V).all()
    for b in range(blocks):                                                        # a block lists each of its vertices once
        mine = ids[first[b]:first[b + 1]]
        assert len(np.unique(mine)) == len(mine)
        assert set(mine.tolist()) == set(faces[b * TRIS:(b + 1) * TRIS].reshape(-1).tolist())


@pytest.mark.parametrize("k", [1, 5])
def test_shared_vertex_grid_with_a_tail_block(k):
    faces, V = grid(40, 23, 256 * k + 37)
    has, first, ids, tris = build(faces, V)
    assert has and len(first) == k + 2
    check_tables(faces, V, first, ids, tris)
    assert first[-1] - first[-2] <= 3 * 37                                         # the tail block lists only its own vertices
    assert np.diff(first.astype(np.int64))[:-1].max() < 256                        # a grid block shares most of its vertices


def test_a_mesh_smaller_than_one_block():
    faces, V = grid(6, 5)
    has, first, ids, tris = build(faces, V)
    assert has and len(first) == 2
    check_tables(faces, V, first, ids, tris)


def test_a_soup_over_the_cap_has_no_meshlets():
    F = 700
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)                         # 768 distinct vertices per block of 256
    has, _, ids, _ = build(faces, 3 * F)
    assert not has and len(ids) == 0
    # (the same soup with 128 distinct vertices per block is fine: the decision is the cap's, not the sharing's)
    has, first, ids, tris = build(faces % 128 + 128 * (np.arange(F)[:, None] // TRIS), 3 * F)
    assert has
    check_tables(faces % 128 + 128 * (np.arange(F)[:, None] // TRIS), 3 * F, first, ids, tris)


@pytest.mark.parametrize("bad", ["V", -1])
def test_one_index_out_of_range_has_no_meshlets(bad):
    faces, V = grid(20, 10)
    faces = faces.copy()
    faces[301, 1] = V if bad == "V" else -1
    has, _, _, _ = build(faces, V)
    assert not has
    faces[301, 1] = V - 1
    has, first, ids, tris = build(faces, V)
    assert has
    check_tables(faces, V, first, ids, tris)


def test_the_fallback_is_per_mesh_not_per_block():
    """One block over the cap among many that are not: the whole mesh reports no meshlets."""
    faces, V = grid(40, 23, 256 * 4)
    faces = faces.copy()
    faces[256:512] = np.arange(V, V + 768, dtype=np.int32).reshape(256, 3)
    has, _, _, _ = build(faces, V + 768)
    assert not has


def test_bad_arguments_are_refused():
    from semantic_meshes_amd import _lib
    faces, V = grid(6, 5)
    first, tris, ids = np.zeros(2, np.uint32), np.zeros(len(faces), np.uint32), np.zeros(4, np.uint32)
    used, has = ctypes.c_uint64(0), ctypes.c_int(0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    L = _lib.lib()
    assert L.smesh_meshlets_build(p(faces), len(faces), V, p(first), p(ids), len(ids), p(tris), ctypes.byref(used), ctypes.byref(has)) == _lib.ERR_INVALID   # too small
    assert L.smesh_meshlets_build(None, len(faces), V, p(first), p(ids), len(ids), p(tris), ctypes.byref(used), ctypes.byref(has)) == _lib.ERR_INVALID


def test_extension_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    from semantic_meshes_amd import _lib
    ext = _declared(HEADER)
    assert ext == sorted(["smesh_meshlets_build", "smesh_last_raster_path"])
    assert sorted(_lib.MESHLET_SIGNATURES) == ext
    assert not set(ext) & set(_declared(os.path.join(ROOT, "include", "smesh.h")))
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+SMESH_MESHLET_TRIS\s+(\d+)", text).group(1)) == _lib.MESHLET_TRIS == TRIS
    assert int(re.search(r"#define\s+SMESH_MESHLET_MAX_VERTS\s+(\d+)", text).group(1)) == _lib.MESHLET_MAX_VERTS == CAP
    assert _lib.lib().smesh_last_raster_path() in (b"none", b"meshlets", b"vertex-stage")


def test_the_option_exists_and_round_trips():
    from semantic_meshes_amd import _lib
    before = _lib.get_option("raster_meshlets")
    assert before in (0, 1)
    try:
        for v in (0, 1, 0):
            _lib.set_option("raster_meshlets", v)
            assert _lib.get_option("raster_meshlets") == v
    finally:
        _lib.set_option("raster_meshlets", before)


def test_builder_under_sanitizers(tmp_path):
    """tests/meshlets_driver.cpp + meshlets.cpp as ONE stand-alone host program with -fsanitize=address,undefined: run here, on the CPU."""
    exe = str(tmp_path / "meshlets_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "meshlets_driver.cpp"), os.path.join(CSRC, "meshlets.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "meshlets driver ok" in out.stdout
