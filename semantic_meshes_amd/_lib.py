"""ctypes loader for the HIP library (semantic_meshes_amd/csrc/libsmesh_hip.so).

The C ABI is declared in include/smesh.h.  There is deliberately NO CPU fallback here: if the
HIP library is missing or no GPU is usable, calls raise -- the product never routes through oracle/.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMESH_LIB_PATH") or os.path.join(_HERE, "csrc", "libsmesh_hip.so")   # (SMESH_LIB_PATH: a development build, e.g. a copy of csrc/ built with other flags)

OK, ERR_INVALID, ERR_RUNTIME, ERR_NODEVICE = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
IDX_U32, IDX_I32, IDX_U64, IDX_I64 = 0, 1, 2, 3
AGG_KINDS = {"Sum": 0, "Summax": 1, "Mul": 2}
PROF_FUSE_SCATTER, PROF_FUSE_HIST, PROF_RASTER, PROF_FINALIZE, PROF_EXCHANGE = 0, 1, 2, 3, 4

c_void_p, c_int, c_u64, c_u32, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float
P = ctypes.POINTER


class CameraPOD(ctypes.Structure):
    """smesh_camera_t (include/smesh.h)."""
    _fields_ = [
        ("rotation", ctypes.c_float * 9),
        ("translation", ctypes.c_float * 3),
        ("focal", ctypes.c_double * 2),
        ("principal", ctypes.c_double * 2),
        ("width", ctypes.c_uint64),
        ("height", ctypes.c_uint64),
    ]


# name -> (restype, argtypes); one entry per symbol declared in include/smesh.h
SIGNATURES = {
    "smesh_backend": (ctypes.c_char_p, []),
    "smesh_last_error": (ctypes.c_char_p, []),
    "smesh_device_count": (c_int, [P(c_int)]),
    "smesh_synchronize": (c_int, [c_int]),
    "smesh_stream_wait": (c_int, [c_int, c_void_p]),
    "smesh_stream_release": (c_int, [c_int, c_void_p]),
    "smesh_stream_handle": (c_int, [c_int, P(c_void_p)]),
    "smesh_token_record": (c_int, [c_int, P(c_u64)]),
    "smesh_token_done": (c_int, [c_int, c_u64, P(c_int)]),
    "smesh_stream_mark": (c_int, [c_int, c_int]),
    "smesh_stream_mark_elapsed": (c_int, [c_int, c_int, c_int, P(ctypes.c_double)]),
    "smesh_renderer_create_triangles": (c_int, [c_void_p, c_u64, c_void_p, c_u64, c_int, P(c_void_p)]),
    "smesh_renderer_create_texels": (c_int, [c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_u64, c_float, c_int, P(c_void_p)]),
    "smesh_renderer_destroy": (c_int, [c_void_p]),
    "smesh_renderer_num_primitives": (c_int, [c_void_p, P(c_u64)]),
    "smesh_renderer_texel_layout": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "smesh_renderer_render": (c_int, [c_void_p, P(CameraPOD), c_void_p, c_void_p]),
    "smesh_renderer_render_device": (c_int, [c_void_p, P(CameraPOD), P(c_void_p), P(c_void_p)]),
    "smesh_renderer_release_image": (c_int, [c_void_p, c_void_p, c_void_p]),
    "smesh_aggregator_create": (c_int, [c_u64, c_u32, c_int, c_float, c_int, P(c_void_p)]),
    "smesh_aggregator_destroy": (c_int, [c_void_p]),
    "smesh_aggregator_reset": (c_int, [c_void_p]),
    "smesh_aggregator_add": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                     c_void_p, P(ctypes.c_int64), c_int,
                                     c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_aggregator_add_async": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                           c_void_p, P(ctypes.c_int64), c_int,
                                           c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_aggregator_add_many": (c_int, [c_void_p, c_u64, P(c_void_p), c_int, P(ctypes.c_int64), c_int,
                                          P(c_void_p), P(ctypes.c_int64), c_int,
                                          P(c_void_p), P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_aggregator_add_rendered": (c_int, [c_void_p, c_void_p, c_void_p,
                                              c_void_p, P(ctypes.c_int64), c_int,
                                              c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_aggregator_get": (c_int, [c_void_p, c_void_p, c_int]),
    "smesh_aggregator_get_rows": (c_int, [c_void_p, c_u64, c_u64, c_void_p, c_int]),
    "smesh_aggregator_get_raw": (c_int, [c_void_p, c_void_p, c_int]),
    "smesh_aggregator_set_raw": (c_int, [c_void_p, c_void_p, c_int]),
    "smesh_aggregator_raw_pointer": (c_int, [c_void_p, P(c_void_p), P(c_u64)]),
    "smesh_aggregator_row_stride": (c_int, [c_void_p, P(c_u32)]),
    "smesh_comm_unique_id": (c_int, [c_void_p]),
    "smesh_comm_create": (c_int, [c_int, c_int, c_int, c_void_p, P(c_void_p)]),
    "smesh_comm_create_all": (c_int, [P(c_int), c_int, P(c_void_p)]),
    "smesh_comm_destroy": (c_int, [c_void_p]),
    "smesh_comm_rank": (c_int, [c_void_p, P(c_int), P(c_int)]),
    "smesh_allreduce": (c_int, [P(c_void_p), P(c_void_p), c_int]),
    "smesh_reduce_scatter": (c_int, [c_void_p, c_void_p, P(c_u64), P(c_u64)]),
    "smesh_fuse_views_begin": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, P(c_void_p), P(c_void_p), c_int, c_int, P(c_u64), P(c_u64)]),
    "smesh_fuse_views_continue": (c_int, [c_void_p, c_void_p, c_int, P(c_u64), P(c_u64)]),
    "smesh_allreduce_rows": (c_int, [c_void_p, c_void_p, c_u64, c_u64]),
    "smesh_exchange_join": (c_int, [c_void_p]),
    "smesh_aggregator_get_raw_rows": (c_int, [c_void_p, c_u64, c_u64, c_int, c_void_p, c_int]),
    "smesh_aggregator_set_raw_rows": (c_int, [c_void_p, c_u64, c_u64, c_int, c_void_p, c_int]),
    "smesh_comm_allreduce_f64": (c_int, [c_void_p, P(ctypes.c_double), c_int, c_int]),
    "smesh_aggregator_renderer": (c_int, [c_void_p, P(c_void_p)]),
    "smesh_annotation_renderer_render": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int, c_void_p, c_void_p, c_int, c_u64, c_u64]),
    "smesh_annotation_renderer_destroy": (c_int, [c_void_p]),
    "smesh_fuse_view": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_void_p, c_void_p, c_int]),
    "smesh_fuse_views": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), P(c_void_p), c_int]),
    "smesh_aggregator_add_matched": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                             c_void_p, P(ctypes.c_int64), c_int,
                                             c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64, P(c_int)]),
    "smesh_renderer_seal_render": (c_int, [c_void_p, c_void_p]),
    "smesh_renderer_render_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "smesh_box_extent_bound": (c_int, [c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_void_p]),
    "smesh_last_fuse_kernel": (ctypes.c_char_p, []),
    "smesh_last_add_path": (ctypes.c_char_p, []),
    "smesh_profile_enable": (c_int, [c_int, c_int]),
    "smesh_profile_sample_every": (c_int, [c_int, ctypes.c_uint32]),
    "smesh_profile_read": (c_int, [c_int, c_int, P(ctypes.c_double), P(c_u64)]),
    "smesh_profile_read_ex": (c_int, [c_int, c_int, P(ctypes.c_double), P(c_u64), P(c_u64), P(c_u64)]),
    "smesh_profile_regions": (c_int, [c_int, c_int, P(c_u64)]),
    "smesh_profile_reset": (c_int, [c_int]),
    "smesh_synth_probs": (c_int, [c_void_p, c_u64, c_u32, c_u64, c_float, c_int, c_int]),
    "smesh_device_malloc": (c_int, [c_int, c_u64, P(c_void_p)]),
    "smesh_device_free": (c_int, [c_int, c_void_p]),
    "smesh_device_trim": (c_int, [c_int, P(c_u64)]),
    "smesh_set_option": (c_int, [ctypes.c_char_p, ctypes.c_int64]),
    "smesh_get_option": (c_int, [ctypes.c_char_p, P(ctypes.c_int64)]),
    "smesh_host_malloc": (c_int, [c_u64, P(c_void_p)]),
    "smesh_host_free": (c_int, [c_void_p]),
    "smesh_memcpy": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_meshlets.h: the grouped rasteriser's per-block vertex
# tables (built on the host, no device needed) and which path its last launch took; product-only like the tables below
MESHLET_SIGNATURES = {
    "smesh_meshlets_build": (c_int, [c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_u64, c_void_p, P(c_u64), P(c_int)]),
    "smesh_last_raster_path": (ctypes.c_char_p, []),
}
MESHLET_TRIS, MESHLET_MAX_VERTS = 256, 384      # SMESH_MESHLET_TRIS / SMESH_MESHLET_MAX_VERTS

# Label dtypes of include/smesh_labels.h (SMESH_LBL_*), by numpy dtype string
LBL_CODES = {"uint8": 0, "int8": 1, "uint16": 2, "int16": 3, "uint32": 4, "int32": 5, "uint64": 6, "int64": 7}

# Modes of include/smesh_vertices.h (SMESH_VTX_*)
VTX_SUMS, VTX_ANNOTATIONS = 0, 1

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_labels.h: the label-image entry points, a product-only
# extension of the ABI that the CPU oracle does not implement (which is why they are not in SIGNATURES)
EXT_SIGNATURES = {
    "smesh_fuse_view_labels": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_void_p, c_int, P(ctypes.c_int64), c_void_p, c_int]),
    "smesh_fuse_views_labels": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(ctypes.c_int64), P(c_void_p), c_int]),
    "smesh_aggregator_add_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                            c_void_p, c_int, P(ctypes.c_int64), c_int,
                                            c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64]),
}

# Class-vector dtypes of include/smesh_half.h (SMESH_PROBS_*)
PROBS_F32, PROBS_F16, PROBS_BF16 = 0, 1, 2
PROBS_NAMES = {PROBS_F32: "float32", PROBS_F16: "float16", PROBS_BF16: "bfloat16"}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_half.h: float16 / bfloat16 class-vector images,
# product-only like the label entry points
HALF_SIGNATURES = {
    "smesh_fuse_view_probs16": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_void_p, c_int, c_void_p, c_int]),
    "smesh_fuse_views_probs16": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(c_void_p), c_int]),
    "smesh_aggregator_add_probs16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                             c_void_p, c_int, P(ctypes.c_int64), c_int,
                                             c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_narrow_probs": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_vertices.h: the per-vertex results, product-only like
# the label entry points (a table of its own: tests/test_labels_host.py pins EXT_SIGNATURES to the symbols of smesh_labels.h)
VERTEX_SIGNATURES = {
    "smesh_vertex_map_create": (c_int, [c_void_p, c_u64, c_u64, c_int, P(c_void_p)]),
    "smesh_vertex_map_destroy": (c_int, [c_void_p]),
    "smesh_vertex_map_size": (c_int, [c_void_p, P(c_u64), P(c_u64), P(c_u64)]),
    "smesh_vertex_map_adjacency": (c_int, [c_void_p, c_void_p, c_void_p]),
    "smesh_vertex_map_gather": (c_int, [c_void_p, c_void_p, c_int, c_u32, c_int, c_float, c_void_p, c_void_p, c_int]),
    "smesh_aggregator_vertex_annotations": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int]),
    "smesh_renderer_texel_face_rows": (c_int, [c_void_p, c_void_p, c_int, c_u32, c_int, c_float, c_void_p, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_eval.h: confusion matrices and primitive labels,
# product-only like the tables above
PROF_CONFUSION = 5
EVAL_SIGNATURES = {
    "smesh_confusion_create": (c_int, [c_u32, c_int, P(c_void_p)]),
    "smesh_confusion_destroy": (c_int, [c_void_p]),
    "smesh_confusion_reset": (c_int, [c_void_p]),
    "smesh_confusion_get": (c_int, [c_void_p, c_void_p, P(c_u64)]),
    "smesh_confusion_add_counts": (c_int, [c_void_p, c_void_p, c_u64]),
    "smesh_confusion_add_labels": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_u64]),
    "smesh_aggregator_labels": (c_int, [c_void_p, c_float, c_void_p, c_int]),
    "smesh_confusion_add_image": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int, c_void_p, c_u64, c_int,
                                          c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64]),
    "smesh_confusion_add_view": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_void_p, c_u64, c_void_p, c_int, P(ctypes.c_int64), c_int]),
    "smesh_confusion_add_views": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, c_void_p, c_u64, P(c_void_p), c_int,
                                          P(ctypes.c_int64), c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_label_images.h: the fused mesh rendered back into the
# views as label and colour images, product-only like the tables above
PROF_LABEL_IMAGES = 6
LAYOUT_WH, LAYOUT_HW = 0, 1
LABEL_IMAGE_SIGNATURES = {
    "smesh_label_renderer_create": (c_int, [c_void_p, c_u64, c_int, c_u32, c_int, c_u32, c_void_p, c_void_p, c_int, P(c_void_p)]),
    "smesh_label_renderer_destroy": (c_int, [c_void_p]),
    "smesh_label_renderer_render_image": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_int,
                                                  c_void_p, c_void_p, c_int]),
    "smesh_label_renderer_render_views": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, c_int, P(c_void_p), P(c_void_p), c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_probs_labels.h: the labels of a class-vector image and
# their confusion matrix, product-only like the tables above
PROF_PROBS_LABELS = 7
PROBS_LABELS_SIGNATURES = {
    "smesh_probs_labels": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_u32, c_float,
                                   c_void_p, c_int, P(ctypes.c_int64), ctypes.c_int64, c_int, c_int]),
    "smesh_confusion_add_probs": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                          c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_float,
                                          c_void_p, c_int, P(ctypes.c_int64), ctypes.c_int64]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_resize.h: class-vector images resampled from the
# network's resolution to the camera's, their labels and their confusion matrix, product-only like the tables above (no profile slot)
RESIZE_BILINEAR = 1
RESIZE_MODES = {"bilinear": RESIZE_BILINEAR}
RESIZE_SIGNATURES = {
    "smesh_resize_probs": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_u32,
                                   c_void_p, c_int, c_u64, c_u64, c_int, c_int]),
    "smesh_resize_probs_labels": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_u32, c_float,
                                          c_void_p, c_int, P(ctypes.c_int64), ctypes.c_int64, c_u64, c_u64, c_int, c_int]),
    "smesh_confusion_add_probs_resized": (c_int, [c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64,
                                                  c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_float, c_int,
                                                  c_void_p, c_int, P(ctypes.c_int64), ctypes.c_int64]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_sampled.h: (w,h,C) class vectors sampled inside the
# fusion kernel, product-only like the tables above
SAMPLED_SIGNATURES = {
    "smesh_fuse_views_sampled": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(ctypes.c_int64), c_u64, c_u64,
                                         P(c_void_p), c_int, c_int]),
    "smesh_fuse_view_sampled": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_void_p, c_int, P(ctypes.c_int64), c_u64, c_u64,
                                        c_void_p, c_int, c_int]),
    "smesh_aggregator_add_sampled": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(ctypes.c_int64), c_int,
                                             c_void_p, c_int, P(ctypes.c_int64), c_int,
                                             c_void_p, P(ctypes.c_int64), c_int, c_u64, c_u64, c_u64, c_u64, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_label_prep.h: label images at their own resolution and
# in the dataset's ids, product-only like the tables above.  Each prepared entry point is its EXT_SIGNATURES counterpart plus
# (w, h, map, map_len, map_memkind).
LABEL_PREP_MAP_LDS_MAX = 4096      # SMESH_LABEL_PREP_MAP_LDS_MAX
_PREP_TAIL = [c_u64, c_u64, c_void_p, c_u64, c_int]
LABEL_PREP_SIGNATURES = {
    "smesh_labels_prepare": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_void_p, c_u64, c_int, c_u32,
                                     c_void_p, c_int, c_u64, c_u64, c_int]),
    "smesh_fuse_views_labels_prepared": (c_int, EXT_SIGNATURES["smesh_fuse_views_labels"][1] + _PREP_TAIL),
    "smesh_fuse_view_labels_prepared": (c_int, EXT_SIGNATURES["smesh_fuse_view_labels"][1] + _PREP_TAIL),
    "smesh_aggregator_add_labels_prepared": (c_int, EXT_SIGNATURES["smesh_aggregator_add_labels"][1] + _PREP_TAIL),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_label_colors.h: label images that are colour images,
# product-only like the tables above.  Each fusion entry point is its EXT_SIGNATURES counterpart (with three label strides) plus
# (w, h, channels, keys, classes, K).
LABEL_COLORS_LDS_MAX = 4096        # SMESH_LABEL_COLORS_LDS_MAX
_COLORS_TAIL = [c_u64, c_u64, c_int, c_void_p, c_void_p, c_u64]
LABEL_COLORS_SIGNATURES = {
    "smesh_colors_unique": (c_int, [P(c_void_p), c_u64, c_int, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_void_p, c_u64, c_void_p, c_int]),
    "smesh_labels_prepare_colors": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_void_p, c_void_p, c_u64, c_u32,
                                            c_void_p, c_int, c_u64, c_u64, c_int]),
    "smesh_fuse_views_labels_colors": (c_int, EXT_SIGNATURES["smesh_fuse_views_labels"][1] + _COLORS_TAIL),
    "smesh_fuse_view_labels_colors": (c_int, EXT_SIGNATURES["smesh_fuse_view_labels"][1] + _COLORS_TAIL),
    "smesh_aggregator_add_labels_colors": (c_int, EXT_SIGNATURES["smesh_aggregator_add_labels"][1] + _COLORS_TAIL),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_points.h: the closest face of arbitrary points and the
# fused rows of those faces, product-only like the tables above (no profile slot; the modes are SMESH_VTX_*)
POINTS_SIGNATURES = {
    "smesh_surface_index_create": (c_int, [c_void_p, c_u64, c_void_p, c_u64, c_int, P(c_void_p)]),
    "smesh_surface_index_destroy": (c_int, [c_void_p]),
    "smesh_surface_index_stats": (c_int, [c_void_p, P(c_u64), P(c_u32), P(c_u64), P(c_u64)]),
    "smesh_surface_index_nearest": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_float, c_void_p, c_void_p, c_int]),
    "smesh_point_gather": (c_int, [c_void_p, c_int, c_u64, c_u32, c_void_p, c_u64, c_int, c_int, c_float, c_void_p, c_void_p, c_int]),
    "smesh_aggregator_point_annotations": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_int, c_float, c_void_p, c_void_p, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_depth.h: fusion gated by sensor depth, product-only like
# the tables above (no profile slot)
DEPTH_U16, DEPTH_F32 = 0, 1                                         # SMESH_DEPTH_*
DEPTH_IMG_LABELS_U8, DEPTH_IMG_LABELS_U16 = 3, 4                    # SMESH_DEPTH_IMG_* (class vectors: the SMESH_PROBS_* codes)


class DepthGatePOD(ctypes.Structure):
    """smesh_depth_gate_t (include/smesh_depth.h)."""
    _fields_ = [("scale", c_float), ("abs_tol", c_float), ("rel_tol", c_float), ("max_depth", c_float), ("missing_keep", ctypes.c_int32)]


DEPTH_SIGNATURES = {
    "smesh_depth_weights": (c_int, [c_void_p, c_u64, c_u64, c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64,
                                    P(DepthGatePOD), c_void_p, c_void_p, c_void_p, c_int]),
    "smesh_fuse_views_depth": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(c_void_p),
                                       P(c_void_p), c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, P(DepthGatePOD), c_void_p]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_view_weights.h: fusion weighted by viewing geometry,
# product-only like the tables above (no profile slot; image kinds and sensor arguments are those of smesh_depth.h)
VW_MAX_POWER = 16                                                   # SMESH_VW_MAX_POWER


class ViewWeightsPOD(ctypes.Structure):
    """smesh_view_weights_spec_t (include/smesh_view_weights.h)."""
    _fields_ = [("power", ctypes.c_int32), ("min_cos", c_float), ("two_sided", ctypes.c_int32), ("max_depth", c_float), ("falloff_depth", c_float)]


VIEW_WEIGHTS_SIGNATURES = {
    "smesh_view_weights": (c_int, [c_void_p, P(CameraPOD), c_void_p, c_void_p, c_u64, c_u64, P(ViewWeightsPOD), c_void_p, c_void_p, c_void_p]),
    "smesh_fuse_views_view_weights": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(c_void_p), P(ViewWeightsPOD),
                                              P(c_void_p), c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, P(DepthGatePOD), c_void_p, c_void_p]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_edge_gate.h: fusion gated at occlusion edges from the
# rendered depth plane, product-only like the tables above (no profile slot; image kinds and sensor arguments are those of smesh_depth.h)
EDGE_MAX_RADIUS = 8                                                 # SMESH_EDGE_MAX_RADIUS
EDGE_TILE_X, EDGE_TILE_Y = 32, 64                                   # SMESH_EDGE_TILE_X / _Y: the tile of one workgroup of k_edge_weights


class EdgeGatePOD(ctypes.Structure):
    """smesh_edge_gate_t (include/smesh_edge_gate.h)."""
    _fields_ = [("radius", ctypes.c_int32), ("abs_tol", c_float), ("rel_tol", c_float), ("behind", ctypes.c_int32), ("front", ctypes.c_int32),
                ("silhouette", ctypes.c_int32)]


EDGE_GATE_SIGNATURES = {
    "smesh_edge_weights": (c_int, [c_void_p, c_u64, c_u64, P(EdgeGatePOD), c_void_p, c_void_p, c_void_p, c_int]),
    "smesh_fuse_views_weighted": (c_int, [c_void_p, c_void_p, P(CameraPOD), c_u64, P(c_void_p), c_int, P(c_void_p), P(ViewWeightsPOD), P(EdgeGatePOD),
                                          P(c_void_p), c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, P(DepthGatePOD), c_void_p, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_face_graph.h: the faces across every face's edges and the
# propagation of fused rows over them, product-only like the tables above (no profile slot; the output modes are SMESH_VTX_*)
FG_SMOOTH, FG_FILL = 0, 1                                           # SMESH_FG_*
FG_MAX_POWER = 16                                                   # SMESH_FG_MAX_POWER
_FG_TAIL = [c_void_p, c_int, c_int, c_u32, c_float, c_float, c_int, c_float, c_void_p, c_void_p, P(c_u64), c_int]
FACE_GRAPH_SIGNATURES = {
    "smesh_face_graph_create": (c_int, [c_void_p, c_u64, c_u64, c_int, P(c_void_p)]),
    "smesh_face_graph_destroy": (c_int, [c_void_p]),
    "smesh_face_graph_size": (c_int, [c_void_p, P(c_u64), P(c_u64), P(c_u64)]),
    "smesh_face_graph_adjacency": (c_int, [c_void_p, c_void_p, c_void_p]),
    "smesh_face_graph_propagate": (c_int, [c_void_p, c_void_p, c_int, c_u32] + _FG_TAIL),
    "smesh_aggregator_face_propagate": (c_int, [c_void_p, c_void_p] + _FG_TAIL),
    "smesh_face_graph_normal_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_u32, c_int, c_void_p, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_face_segments.h: the connected components of a labelled
# mesh over the face graph and the removal of the small ones, product-only like the tables above (no profile slot)
FACE_SEGMENTS_SIGNATURES = {
    "smesh_face_segments_create": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, P(c_void_p)]),
    "smesh_aggregator_face_segments": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_int, c_float, P(c_void_p)]),
    "smesh_face_segments_destroy": (c_int, [c_void_p]),
    "smesh_face_segments_size": (c_int, [c_void_p, P(c_u64), P(c_u64), P(c_u64)]),
    "smesh_face_segments_get": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "smesh_face_segments_despeckle_labels": (c_int, [c_void_p, c_u32, c_void_p, c_int, P(c_u64), P(c_u64)]),
    "smesh_face_segments_despeckle_rows": (c_int, [c_void_p, c_u32, c_void_p, c_int, c_u32, c_void_p, c_int]),
    "smesh_aggregator_face_segments_despeckle": (c_int, [c_void_p, c_void_p, c_u32, c_void_p, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_segment_stats.h: fused rows and areas pooled over the
# segments, and the despeckle by a per-segment measure, product-only like the tables above (no profile slot)
_SS_POOL_TAIL = [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int]      # face weights, their memkind, mode, threshold, outs
SEGMENT_STATS_SIGNATURES = {
    "smesh_segment_stats_face_areas": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "smesh_segment_stats_members": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "smesh_segment_stats_pool": (c_int, [c_void_p, c_void_p, c_int, c_u32] + _SS_POOL_TAIL),
    "smesh_segment_stats_pool_faces": (c_int, [c_void_p, c_void_p, c_int, c_u32] + _SS_POOL_TAIL),
    "smesh_aggregator_segment_stats_pool": (c_int, [c_void_p, c_void_p] + _SS_POOL_TAIL),
    "smesh_aggregator_segment_stats_pool_faces": (c_int, [c_void_p, c_void_p] + _SS_POOL_TAIL),
    "smesh_segment_stats_despeckle_labels": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_int, P(c_u64), P(c_u64)]),
    "smesh_segment_stats_despeckle_rows": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_int, c_u32, c_void_p, c_int]),
    "smesh_aggregator_segment_stats_despeckle": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_int]),
}

# name -> (restype, argtypes); one entry per symbol declared in include/smesh_lens.h: images from cameras with lens distortion,
# undistorted on the device, product-only like the tables above (no profile slot)
LENS_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")     # COLMAP's polynomial models, subsets of FULL_OPENCV


class LensPOD(ctypes.Structure):
    """smesh_lens_t (include/smesh_lens.h)."""
    _fields_ = [("focal", ctypes.c_double * 2), ("principal", ctypes.c_double * 2), ("k", ctypes.c_double * 6), ("p", ctypes.c_double * 2),
                ("width", ctypes.c_uint64), ("height", ctypes.c_uint64)]


LENS_SIGNATURES = {
    "smesh_undistort_probs": (c_int, [c_void_p, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, c_u32, P(LensPOD), P(CameraPOD),
                                      c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int]),
    "smesh_undistort_pixels": (c_int, [c_void_p, c_int, c_int, P(ctypes.c_int64), c_int, c_u64, c_u64, P(LensPOD), P(CameraPOD),
                                       c_void_p, c_void_p, c_void_p, c_int]),
}

_lib = None
_lock = threading.Lock()


def _elf_dynamic_strings(path):
    """(SONAME or None, [DT_NEEDED ...]) of a little-endian ELF64 shared object, read from its PT_DYNAMIC segment through the program
    headers (section headers may be stripped).  Raises ValueError on anything that is not such a file, truncated ones included."""
    import struct
    with open(path, "rb") as f:
        data = f.read()
    try:
        if data[:6] != b"\x7fELF\x02\x01":
            raise ValueError("not a little-endian ELF64 file")
        phoff, = struct.unpack_from("<Q", data, 0x20)
        phentsize, phnum = struct.unpack_from("<HH", data, 0x36)
        loads, dyn = [], None
        for k in range(phnum):
            typ, flags, off, vaddr, paddr, filesz, memsz, align = struct.unpack_from("<IIQQQQQQ", data, phoff + k * phentsize)
            if typ == 1:
                loads.append((vaddr, off, filesz))
            elif typ == 2:
                dyn = (off, filesz)
        if dyn is None:
            return None, []
        entries = []
        for e in range(dyn[0], dyn[0] + dyn[1], 16):
            tag, val = struct.unpack_from("<qQ", data, e)
            if tag == 0:
                break
            entries.append((tag, val))
        strtab = next((v for t, v in entries if t == 5), None)        # DT_STRTAB: a virtual address
        if strtab is None:
            return None, []
        stroff = next((off + strtab - vaddr for vaddr, off, filesz in loads if vaddr <= strtab < vaddr + filesz), None)
        if stroff is None:
            raise ValueError("DT_STRTAB outside every PT_LOAD segment")

        def cstr(o):
            end = data.index(b"\0", stroff + o)
            return data[stroff + o:end].decode()

        soname, needed = None, []
        for tag, val in entries:
            if tag == 1:
                needed.append(cstr(val))
            elif tag == 14:
                soname = cstr(val)
        return soname, needed
    except (struct.error, IndexError, UnicodeDecodeError) as e:
        raise ValueError("malformed ELF file %s: %s" % (path, e))


def _preload_note(msg):
    """Why the torch-bundled HIP runtime was NOT mapped first (SMESH_DEBUG=1 prints it; a process that later imports torch against
    a second runtime sees no GPU there -- this is the first thing to look at)."""
    global PRELOAD_NOTE
    PRELOAD_NOTE = msg
    if os.environ.get("SMESH_DEBUG"):
        import sys
        print("semantic_meshes_amd: " + msg, file=sys.stderr)


PRELOAD_NOTE = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels ship their own libamdhip64 / libhsa-runtime64 next to torch; a
    process that first loads this library against the system ROCm and later imports torch ends up with TWO runtimes, and
    the second one sees no usable GPU (`torch.cuda.is_available()` False, a hang at exit).  The other order is fine: the
    dynamic linker satisfies our DT_NEEDED `libamdhip64.so.N` with the copy torch already mapped -- IF that copy's SONAME
    is the same `libamdhip64.so.N`.  So, when a torch installation exists in this environment (located, NOT imported) AND
    its bundled runtime carries exactly the SONAME this library was linked against, that runtime is mapped first and both
    then share it in any import order.  A wheel built against another ROCm major (its SONAME differs) is left alone: the
    linker could not reuse it, and mapping it would CREATE the two-runtime state for processes that never import torch.
    SMESH_HIP_RUNTIME=system keeps the system ROCm unconditionally; =<directory> takes libamdhip64.so / libhsa-runtime64.so
    from there (same SONAME check)."""
    import importlib.util
    import sys
    choice = os.environ.get("SMESH_HIP_RUNTIME", "auto")
    if choice == "system" or "torch" in sys.modules:
        return
    libdir = choice if choice not in ("auto", "torch") else None
    if libdir is None:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is None or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    hip = os.path.join(libdir, "libamdhip64.so")
    if not os.path.exists(hip):
        return
    try:
        wanted = [n for n in _elf_dynamic_strings(LIB_PATH)[1] if n.startswith("libamdhip64.so")]
        offered = _elf_dynamic_strings(hip)[0]
    except (OSError, ValueError) as e:
        _preload_note("HIP runtime preload skipped: %s" % e)
        return
    if not wanted or offered != wanted[0]:
        _preload_note("HIP runtime preload skipped: %s offers SONAME %r, libsmesh_hip.so needs %r" % (hip, offered, wanted[:1]))
        return          # another ROCm major: the linker would map the system runtime beside it anyway
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return
    # ... and the RCCL that goes with that runtime (comm.cpp loads RCCL lazily; torch would otherwise map a second one later)
    rccl = os.path.join(libdir, "librccl.so")
    if os.path.exists(rccl):
        os.environ.setdefault("SMESH_RCCL_LIB", rccl)


def lib():
    """Load libsmesh_hip.so (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "semantic_meshes_amd: %s not found -- build it with `make -C semantic_meshes_amd/csrc` "
                        "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % LIB_PATH)
                _preload_hip_runtime()
                L = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + list(HALF_SIGNATURES.items()) + list(VERTEX_SIGNATURES.items()) + list(EVAL_SIGNATURES.items()) + list(LABEL_IMAGE_SIGNATURES.items()) + list(MESHLET_SIGNATURES.items()) + list(PROBS_LABELS_SIGNATURES.items()) + list(RESIZE_SIGNATURES.items()) + list(SAMPLED_SIGNATURES.items()) + list(LABEL_PREP_SIGNATURES.items()) + list(LABEL_COLORS_SIGNATURES.items()) + list(POINTS_SIGNATURES.items()) + list(DEPTH_SIGNATURES.items()) + list(VIEW_WEIGHTS_SIGNATURES.items()) + list(EDGE_GATE_SIGNATURES.items()) + list(FACE_GRAPH_SIGNATURES.items()) + list(FACE_SEGMENTS_SIGNATURES.items()) + list(SEGMENT_STATS_SIGNATURES.items()) + list(LENS_SIGNATURES.items()):
                    fn = getattr(L, name)  # AttributeError if the library does not export the ABI
                    fn.restype = res
                    fn.argtypes = args
                _lib = L
    return _lib


def check(status):
    """Map a C status to the reference's exception types (ValueError <- std::invalid_argument)."""
    if status == OK:
        return
    msg = lib().smesh_last_error().decode(errors="replace")
    if status == ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def device_count():
    n = c_int(0)
    check(lib().smesh_device_count(ctypes.byref(n)))
    return n.value


_flush_hooks = []      # callables(device): work the Python layer has accepted but not yet handed to the library (fusion.py: deferred views)


def flush_pending(device=None):
    """Hand every deferred view (MeshAggregator.add / fuse_view, fusion.py) of `device` (None: all devices) to the library now."""
    for hook in list(_flush_hooks):
        hook(device)


def last_fuse_kernel():
    """Name of the fusion kernel the calling thread's last add / fuse call used (`smesh_last_fuse_kernel`) -- deferred views
    (fusion.py) are handed to the library first, so that "last call" means the caller's last call."""
    flush_pending()
    return lib().smesh_last_fuse_kernel().decode()


def last_add_path():
    """Which path the calling thread's last add() took (`smesh_last_add_path`); deferred views are handed over first."""
    flush_pending()
    return lib().smesh_last_add_path().decode()


def last_raster_path():
    """Which path the calling thread's last grouped raster launch took (`smesh_last_raster_path`): "meshlets", "vertex-stage" or
    "none"; deferred views are handed over first."""
    flush_pending()
    return lib().smesh_last_raster_path().decode()


RASTER_REPORT_FIELDS = ("kernel", "mode", "views", "tpw", "groups", "chunk", "stages")


def last_raster_instance():
    """Which instance the calling thread's last raster launch was, as a dict of the read-only options "last_raster_kernel" (0 none yet,
    1 k_raster_frag, 2 k_raster_frag_group, 3 k_raster_frag_group_ml, 4 the direct path), "_mode" (the MODE template value: 1 wg_push,
    2 spread waves, 4 texels, 8 packed fragments), "_views", "_tpw", "_groups", "_chunk" and "_stages" (1 a vertex stage ran,
    2 k_raster_medium, 4 k_raster_huge, 8 the resolve wrote depth planes, 16 the packed resolve); deferred views are handed over first."""
    flush_pending()
    return {f: get_option("last_raster_" + f) for f in RASTER_REPORT_FIELDS}


def set_option(name, value):
    """`smesh_set_option`: a run-time option by name (include/smesh.h), e.g. "raster_meshlets"."""
    check(lib().smesh_set_option(name.encode(), int(value)))


def get_option(name):
    """`smesh_get_option`: the value of a run-time option."""
    v = ctypes.c_int64(0)
    check(lib().smesh_get_option(name.encode(), ctypes.byref(v)))
    return v.value


def synchronize(device=0):
    flush_pending(device)
    check(lib().smesh_synchronize(device))
