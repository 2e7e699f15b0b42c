"""Label and colour images of the fused mesh (semantic_meshes_amd/label_images.py, include/smesh_label_images.h), the part that needs
no GPU: the extension header, its ctypes table, and the arguments that are refused before a device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LABEL_IMAGES_HEADER = os.path.join(INCLUDE, "smesh_label_images.h")
HEADER = os.path.join(INCLUDE, "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99():
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", LABEL_IMAGES_HEADER])


def test_declared_functions_have_their_signatures_and_belong_to_no_other_table():
    from semantic_meshes_amd import _lib
    declared = _declared(LABEL_IMAGES_HEADER)
    assert declared == sorted(["smesh_label_renderer_create", "smesh_label_renderer_destroy", "smesh_label_renderer_render_image",
                               "smesh_label_renderer_render_views"])
    assert sorted(_lib.LABEL_IMAGE_SIGNATURES) == declared
    assert not set(declared) & set(_declared(HEADER))              # none of it went into the ABI the oracle implements
    for other in ("smesh_labels.h", "smesh_vertices.h", "smesh_eval.h"):
        assert not set(declared) & set(_declared(os.path.join(INCLUDE, other))), other
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.VERTEX_SIGNATURES) | set(_lib.EVAL_SIGNATURES))


def test_the_library_exports_the_header():
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in _declared(LABEL_IMAGES_HEADER):
        assert name in names, "%s is not exported by libsmesh_hip.so" % name


def test_profile_slot_and_layout_codes():
    from semantic_meshes_amd import _lib
    text = open(LABEL_IMAGES_HEADER).read()
    slot = int(re.search(r"#define\s+SMESH_PROF_LABEL_IMAGES\s+(\d+)", text).group(1))
    slots = int(re.search(r"#define\s+SMESH_PROF_SLOTS\s+(\d+)", open(HEADER).read()).group(1))
    used = {int(v) for v in re.findall(r"#define\s+SMESH_PROF_[A-Z_]+\s+(\d+)\s*/\*", open(HEADER).read())}
    eval_slot = int(re.search(r"#define\s+SMESH_PROF_CONFUSION\s+(\d+)", open(os.path.join(INCLUDE, "smesh_eval.h")).read()).group(1))
    assert slot == _lib.PROF_LABEL_IMAGES and slot < slots and slot not in used and slot != eval_slot
    assert int(re.search(r"#define\s+SMESH_LAYOUT_WH\s+(\d+)", text).group(1)) == _lib.LAYOUT_WH
    assert int(re.search(r"#define\s+SMESH_LAYOUT_HW\s+(\d+)", text).group(1)) == _lib.LAYOUT_HW
    assert _lib.LAYOUT_WH != _lib.LAYOUT_HW


def test_the_reference_package_name_exports_the_same_class():
    import semantic_meshes
    import semantic_meshes_amd
    assert semantic_meshes.fusion.LabelRenderer is semantic_meshes_amd.fusion.LabelRenderer


def test_bad_arguments_are_refused_before_a_device_is_touched(monkeypatch):
    from semantic_meshes_amd import _lib, fusion

    def no_device():
        raise AssertionError("the library was loaded: a device would have been touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    table = np.array([0, 1, -1, 2], np.int32)
    palette = np.arange(19 * 3, dtype=np.uint8).reshape(19, 3)
    L = fusion.LabelRenderer
    bad = [
        lambda: L(table, 0),                                                   # classes <= 0
        lambda: L(table, -3),
        lambda: L(table, 19, palette=palette.astype(np.int32)),                # a palette that is not uint8 [classes, 3]
        lambda: L(table, 19, palette=palette[:18]),
        lambda: L(table, 19, palette=palette.reshape(3, 19)),
        lambda: L(table, 19, palette=palette.ravel()),
        lambda: L(table, 256, dtype=np.uint8),                                 # classes beyond the dtype
        lambda: L(table, 65536),
        lambda: L(table, 65536, dtype=np.uint16),
        lambda: L(table, 19, dtype=np.int32),
        lambda: L(table, 19, dont_care_label=256),                             # a don't-care label the dtype cannot hold
        lambda: L(table, 19, dont_care_label=-1),
        lambda: L(table, 300, dont_care_label=65536),
        lambda: L(table, 19, layout="CHW"),                                    # an unknown layout
        lambda: L(table, 19, layout="hw"),
        lambda: L(table.astype(np.float32), 19),                               # a label table that is not a 1-D integer array
        lambda: L(table.reshape(2, 2), 19),
        lambda: L(np.int32(3), 19),
        lambda: L(table, 19).render_views_colors(None, []),                    # a colour request without a palette
        lambda: L(table, 19).render_views(None, [], colors=True),
        lambda: L(table, 19).render_view(None, None, colors=True),
        lambda: L(table, 19).render_image(np.zeros((4, 4), np.uint32), colors=True),
        lambda: L(table, 19).render_image_colors_device(np.zeros((4, 4), np.uint32)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    # ... and what is accepted, with the defaults the documentation states
    lr = L(table, 19, palette=palette)
    assert lr.dtype == np.uint8 and lr.dont_care_label == 255 and lr.layout == "HW" and lr.primitives == 4
    lr = L(table.astype(np.int64), 300)
    assert lr.dtype == np.uint16 and lr.dont_care_label == 65535
    assert L(table, 255).dtype == np.uint8 and L(table, 256).dtype == np.uint16
    assert L(table, 255, dont_care_label=7).dont_care_label == 7
    assert L(np.zeros(0, np.int32), 1).primitives == 0
