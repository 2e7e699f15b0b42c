"""Per-vertex results (include/smesh_vertices.h, data.Ply.save_vertex_colors), the part that needs no GPU: the extension header and its
ctypes table, and the PLY writer."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTX_HEADER = os.path.join(ROOT, "include", "smesh_vertices.h")
HEADER = os.path.join(ROOT, "include", "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_vertex_header_is_c99_and_the_library_exports_it():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", VTX_HEADER])
    from semantic_meshes_amd import _lib
    declared = _declared(VTX_HEADER)
    assert declared == sorted(["smesh_vertex_map_create", "smesh_vertex_map_destroy", "smesh_vertex_map_size", "smesh_vertex_map_adjacency",
                               "smesh_vertex_map_gather", "smesh_aggregator_vertex_annotations", "smesh_renderer_texel_face_rows"])
    assert sorted(_lib.VERTEX_SIGNATURES) == declared              # every declared symbol has its ctypes signature
    assert not set(declared) & set(_declared(HEADER))              # none of it went into the ABI the oracle implements
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in declared:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    modes = dict(re.findall(r"#define\s+SMESH_VTX_([A-Z]+)\s+(\d+)", open(VTX_HEADER).read()))
    assert (int(modes["SUMS"]), int(modes["ANNOTATIONS"])) == (_lib.VTX_SUMS, _lib.VTX_ANNOTATIONS)


def _parse_ply(path):
    """(vertices float32[V,3], colours uint8[V,3], faces int32[F,3], header lines), by hand."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    header = blob[:end].decode("ascii").splitlines()
    nv = int([l for l in header if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in header if l.startswith("element face")][0].split()[-1])
    body = blob[end:]
    v, c, f = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.uint8), np.empty((nf, 3), np.int32)
    if header[1] == "format ascii 1.0":
        lines = body.decode("ascii").splitlines()
        assert len(lines) == nv + nf
        for i in range(nv):
            tok = lines[i].split()
            assert len(tok) == 6
            v[i], c[i] = [float(t) for t in tok[:3]], [int(t) for t in tok[3:]]
        for i in range(nf):
            tok = [int(t) for t in lines[nv + i].split()]
            assert len(tok) == 4 and tok[0] == 3
            f[i] = tok[1:]
    else:
        assert header[1] == "format binary_little_endian 1.0"
        assert len(body) == nv * 15 + nf * 13
        for i in range(nv):
            rec = struct.unpack_from("<fffBBB", body, i * 15)
            v[i], c[i] = rec[:3], rec[3:]
        for i in range(nf):
            rec = struct.unpack_from("<Biii", body, nv * 15 + i * 13)
            assert rec[0] == 3
            f[i] = rec[1:]
    return v, c, f, header


@pytest.mark.parametrize("binary", [False, True])
def test_save_vertex_colors_round_trip(tmp_path, binary):
    from semantic_meshes_amd import data, synth
    mesh = synth.grid_mesh(7, 5)
    src = str(tmp_path / "in.ply")
    data._write_ply(src, mesh.vertices, mesh.faces, np.zeros((len(mesh.faces), 3), np.uint8), True)
    ply = data.Ply(src)
    rng = np.random.default_rng(3)
    colors = rng.integers(0, 256, size=(len(ply.vertices), 3)).astype(np.uint8)
    out = str(tmp_path / "out.ply")
    ply.save_vertex_colors(out, colors, binary=binary)
    v, c, f, header = _parse_ply(out)
    assert header == ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"),
                      "element vertex %d" % len(ply.vertices), "property float x", "property float y", "property float z",
                      "property uchar red", "property uchar green", "property uchar blue",
                      "element face %d" % len(ply.faces), "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(v.view(np.uint32), ply.vertices.view(np.uint32))
    assert np.array_equal(c, colors) and np.array_equal(f, ply.faces)
    again = data.Ply(out)                                              # ... and the package's own reader takes it
    assert np.array_equal(again.vertices, ply.vertices) and np.array_equal(again.faces, ply.faces)
    face_colors = rng.integers(0, 256, size=(len(ply.faces), 3)).astype(np.uint8)
    ply.save(str(tmp_path / "faces.ply"), face_colors, binary=binary)  # Ply.save is what it was: colours per face
    assert "property uchar red" in open(str(tmp_path / "faces.ply"), "rb").read().split(b"end_header")[0].decode().split("element face")[1]


def test_save_vertex_colors_refuses_wrong_arrays(tmp_path):
    from semantic_meshes_amd import data, synth
    mesh = synth.grid_mesh(4, 2)                                       # (15 vertices, 16 faces)
    src = str(tmp_path / "in.ply")
    data._write_ply(src, mesh.vertices, mesh.faces, np.zeros((len(mesh.faces), 3), np.uint8), False)
    ply = data.Ply(src)
    V = len(ply.vertices)
    for bad in (np.zeros((V, 3), np.int32), np.zeros((V, 3), np.float32), np.zeros((V + 1, 3), np.uint8), np.zeros((V, 4), np.uint8),
                np.zeros(V * 3, np.uint8), np.zeros((len(ply.faces), 3), np.uint8)):
        with pytest.raises(ValueError):
            ply.save_vertex_colors(str(tmp_path / "bad.ply"), bad)
    assert not os.path.exists(str(tmp_path / "bad.ply"))


def test_vertex_transfer_refuses_wrong_faces_before_it_needs_a_device():
    from semantic_meshes_amd import fusion
    for faces, V in ((np.zeros((4, 2), np.int32), 5), (np.zeros((4, 3), np.float32), 5), (np.zeros(12, np.int32), 5),
                     (np.full((4, 3), 5, np.int32), 5), (np.full((4, 3), -1, np.int32), 5), (np.zeros((4, 3), np.int32), -1)):
        with pytest.raises(ValueError):
            fusion.VertexTransfer(faces, V)
