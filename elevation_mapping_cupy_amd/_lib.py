"""ctypes binding of ``libemap_hip.so`` (C ABI: ``include/emap_hip.h``).

The product path has NO CPU fallback: if the shared library is missing, cannot be loaded, or no HIP device
is present, the calls below raise -- they never route to NumPy or to the test oracle.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EMAP_HIP_LIB") or os.path.join(_PKG, "libemap_hip.so")      # (override: A/B runs of two builds)

_INTS = ["cell_n", "mode", "enable_edge_sharpen", "enable_visibility_cleanup", "enable_drift_compensation",
         "enable_overlap_clearance", "dilation_size", "pad_"]
_DOUBLES = [
    "resolution", "sensor_noise_factor", "mahalanobis_thresh", "outlier_variance",
    "drift_compensation_variance_inlier", "traversability_inlier", "wall_num_thresh", "max_ray_length",
    "cleanup_step", "cleanup_cos_thresh", "min_valid_distance", "max_height_range",
    "ramped_height_range_a", "ramped_height_range_b", "ramped_height_range_c", "max_variance",
    "initial_variance", "time_variance", "time_interval", "min_height_drift_cnt",
    "max_drift", "drift_compensation_alpha", "position_noise_thresh", "orientation_noise_thresh",
    "overlap_clear_range_xy", "overlap_clear_range_z", "ray_step", "reserved_",
]


class EmapParams(ct.Structure):
    """struct emap_params (include/emap_hip.h)."""
    _fields_ = ([(n, ct.c_int32) for n in _INTS] + [(n, ct.c_double) for n in _DOUBLES] +
                [("w1", ct.c_float * 36), ("w2", ct.c_float * 36), ("w3", ct.c_float * 36), ("w_out", ct.c_float * 12)])


class EmapStrip(ct.Structure):
    _fields_ = [("row_begin", ct.c_int32), ("row_count", ct.c_int32), ("halo_rows", ct.c_int32), ("pad_", ct.c_int32)]


class EmapStats(ct.Structure):
    _fields_ = [("err_sum", ct.c_double), ("err_cnt", ct.c_uint32), ("gate_fired", ct.c_int32),
                ("mean_error", ct.c_float), ("additive_mean_error", ct.c_float), ("shift", ct.c_float),
                ("n_points", ct.c_uint32), ("ray_visits", ct.c_uint64)]


class EmapSemSpec(ct.Structure):
    _fields_ = [("n_sum", ct.c_int32), ("sum_chan", ct.c_int32 * 16), ("sum_layer", ct.c_int32 * 16), ("sum_kind", ct.c_int32 * 16),
                ("n_col", ct.c_int32), ("col_chan", ct.c_int32 * 4), ("col_layer", ct.c_int32 * 4), ("alpha", ct.c_double)]


class EmapDepthDesc(ct.Structure):
    """struct emap_depth_desc (include/emap_hip.h: emap_bind_depth_image)."""
    _fields_ = ([(n, ct.c_int32) for n in ("height", "width", "depth_dtype", "step", "has_rgb", "n_features")] +
                [(n, ct.c_float) for n in ("fx", "fy", "cx", "cy", "depth_scale", "min_depth", "max_depth", "confidence_threshold")])


class EmapCloudMsgDesc(ct.Structure):
    """struct emap_cloud_msg_desc (include/emap_hip.h: emap_bind_cloud_message)."""
    _fields_ = ([(n, ct.c_int32) for n in ("height", "width", "point_step", "row_step", "is_bigendian", "n_cols")] +
                [("offset", ct.c_int32 * 19), ("conv", ct.c_int32 * 19)])


class EmapImageMsgDesc(ct.Structure):
    """struct emap_image_msg_desc (include/emap_hip.h: emap_input_image_message)."""
    _fields_ = [(n, ct.c_int32) for n in ("height", "width", "step", "elem", "n_chan", "is_bigendian", "swap_rb")]


class EmapImageSpec(ct.Structure):
    """struct emap_image_spec (include/emap_hip.h: emap_input_image_message)."""
    _fields_ = [(n, ct.c_int32) for n in ("kind", "layer", "plane", "pad")] + [("alpha", ct.c_double)]


class EmapGridLayer(ct.Structure):
    """struct emap_grid_layer (include/emap_hip.h: emap_publish_grid_map)."""
    _fields_ = [(n, ct.c_int32) for n in ("kind", "index", "slot")]


class EmapGridLayerEx(ct.Structure):
    """struct emap_grid_layer_ex (include/emap_hip.h: emap_publish_grid_map_ex)."""
    _fields_ = [(n, ct.c_int32) for n in ("kind", "index", "slot", "flags")]


class EmapGridWindow(ct.Structure):
    """struct emap_grid_window (include/emap_hip.h: emap_publish_grid_windows)."""
    _fields_ = [(n, ct.c_int32) for n in ("i0", "j0", "ni", "nj")]


class EmapCloudField(ct.Structure):
    """struct emap_cloud_field (include/emap_hip.h: emap_publish_point_cloud)."""
    _fields_ = [(n, ct.c_int32) for n in ("kind", "index", "flags", "cloud_flags")]


class EmapPlaneParams(ct.Structure):
    """struct emap_plane_params (include/emap_hip.h: emap_plane_segmentation)."""
    _fields_ = ([(n, ct.c_int32) for n in ("kernel_size", "planarity_opening_filter", "min_number_points_per_label", "connectivity",
                                           "use_only_above_for_upper_bound", "reserved")] +
                [("center_z", ct.c_float), ("reserved_f", ct.c_float)] +
                [(n, ct.c_double) for n in ("resolution", "origin_x", "origin_y", "plane_patch_error_threshold", "cos_local_plane_inclination",
                                            "cos_plane_inclination", "global_plane_fit_distance_error_threshold", "cos_global_plane_fit_angle")])


class EmapPlaneRecord(ct.Structure):
    """struct emap_plane_record (include/emap_hip.h: emap_plane_segmentation)."""
    _fields_ = [(n, ct.c_int32) for n in ("label", "n_points", "needs_refinement", "n_left_out")] + [("support", ct.c_double * 3), ("normal", ct.c_double * 3)]


PLANE_RECORD_DTYPE = np.dtype([("label", np.int32), ("n_points", np.int32), ("needs_refinement", np.int32), ("n_left_out", np.int32),
                               ("support", np.float64, (3,)), ("normal", np.float64, (3,))])      # the bytes of emap_plane_record
PLANE_OPEN_MAX = 8                                  # EMAP_PLANE_OPEN_MAX


class EmapTerrainParams(ct.Structure):
    """struct emap_terrain_params (include/emap_hip.h: emap_planar_terrain)."""
    _fields_ = ([(n, ct.c_int32) for n in ("preprocess", "median_kernel_size", "median_repeats", "nonplanar_horizontal_offset", "want", "reserved")] +
                [(n, ct.c_double) for n in ("smoothing_dilation_size", "smoothing_box_kernel_size", "smoothing_gauss_kernel_size",
                                            "extracted_planes_height_offset", "nonplanar_height_offset")])


class EmapTerrainPlanes(ct.Structure):
    """struct emap_terrain_planes (include/emap_hip.h: emap_planar_terrain)."""
    _fields_ = [("plane", ct.POINTER(ct.c_float) * 8)]


TERRAIN_KERNEL_MAX, TERRAIN_OFFSET_MAX, TERRAIN_REPEATS_MAX = 31, 15, 8      # EMAP_TERRAIN_KERNEL_MAX / _OFFSET_MAX / _REPEATS_MAX (caps)
# EMAP_TERRAIN_ELEVATION ..: bit k of `want` asks for plane k
TERRAIN_PLANES = ("elevation", "smooth_planar", "plane_classification", "elevation_before_postprocess",
                  "elevationWithNaN", "elevationWithNaN_i", "elevationWithNaNClosed", "elevationWithNaNClosedDilated")


class EmapRegionParams(ct.Structure):
    """struct emap_region_params (include/emap_hip.h: emap_planar_regions)."""
    _fields_ = [("mode", ct.c_int32), ("margin_size", ct.c_int32), ("reserved", ct.c_int32 * 2)]


class EmapRegionRing(ct.Structure):
    """struct emap_region_ring (include/emap_hip.h: emap_planar_regions)."""
    _fields_ = [(n, ct.c_int32) for n in ("first_vertex", "n_vertices", "image", "is_hole", "label", "root", "crack", "boundary")]


REGION_MARGIN_MAX, REGION_SIDE_MAX, REGION_RAW_SIDE_MAX = 14, 7724, 23170      # EMAP_REGION_MARGIN_MAX / _SIDE_MAX / _RAW_SIDE_MAX (caps)


class EmapPluginOp(ct.Structure):
    """struct emap_plugin_op (include/emap_hip.h: emap_plugin_chain)."""
    _fields_ = [(n, ct.c_int32) for n in ("type", "dst_plane", "src_kind", "src_index", "i0", "i1", "flags")] + [("f0", ct.c_float)]


class EmapPluginSrc(ct.Structure):
    """struct emap_plugin_src (include/emap_hip.h: emap_plugin_chain_ex): one entry of the side table of sources."""
    _fields_ = [(n, ct.c_int32) for n in ("kind", "index", "flags", "reserved")] + [("f0", ct.c_float), ("f1", ct.c_float), ("d0", ct.c_double)]


class EmapPolygonVerdict(ct.Structure):
    """struct emap_polygon_verdict (include/emap_hip.h: emap_polygon_safety)."""
    _fields_ = [("sum_valid", ct.c_double), ("sum_risk", ct.c_double), ("max_risk", ct.c_float)] + \
               [(n, ct.c_int32) for n in ("n_inside", "n_risky", "flags", "row_begin", "n_rows", "col_begin", "n_cols")]


GRID_ORDERS = {"rows": 0, "message": 1}             # EMAP_GRID_ROWS / EMAP_GRID_MESSAGE
GRID_BUILTIN, GRID_SEMANTIC, GRID_NORMAL_COLOR = 0, 1, 2
GRID_MAX_LAYERS = 32                                # EMAP_GRID_MAX_LAYERS
GRID_PLUGIN = 3                                     # EMAP_GRID_PLUGIN: a resident plugin plane (emap_publish_grid_map_ex)
GRID_FILL_NAN, GRID_ADD_Z = 1, 2                    # EMAP_GRID_FILL_NAN / EMAP_GRID_ADD_Z
GRID_MAX_WINDOWS = 64                               # EMAP_GRID_MAX_WINDOWS: windows per emap_publish_grid_windows call (a cap)
CLOUD_POINT, CLOUD_TEST, CLOUD_HIDDEN, CLOUD_NORMAL_MIN, CLOUD_INDEX = 1, 2, 4, 8, 16      # EMAP_CLOUD_*: entry flags (POINT / TEST / HIDDEN), call flags
PLUGIN_MAX_PLANES = PLUGIN_MAX_OPS = 32             # EMAP_PLUGIN_MAX_PLANES / EMAP_PLUGIN_MAX_OPS
PLUGIN_OPS = {"min_filter": 0, "max_filter": 1, "smooth": 2, "erosion": 3, "robot_centric": 4, "inpaint_fronts": 6}      # EMAP_PLUGIN_MIN_FILTER .. (5: unassigned)
PLUGIN_OPS_EX = {"semantic_filter": 7, "semantic_trav": 8, "max_layer": 9, "features_pca": 10}      # EMAP_PLUGIN_SEMANTIC_FILTER ..: the ops of emap_plugin_chain_ex (a run of the side table)
PLUGIN_SRC_LAYER, PLUGIN_SRC_PLANE, PLUGIN_SRC_SEMANTIC = 0, 1, 2      # EMAP_PLUGIN_SRC_*
PLUGIN_REVERSE, PLUGIN_THRESHOLD, PLUGIN_MIN = 1, 2, 4      # EMAP_PLUGIN_REVERSE / EMAP_PLUGIN_THRESHOLD / EMAP_PLUGIN_MIN (op flags)
PLUGIN_SRC_AT_MOST, PLUGIN_SRC_ZERO_DEFAULT, PLUGIN_SRC_REVERSE, PLUGIN_SRC_SCALE, PLUGIN_SRC_THRESHOLD = 1, 2, 4, 8, 16      # flags of a source
PLUGIN_MAX_SRCS = 2048                              # EMAP_PLUGIN_MAX_SRCS
PLUGIN_SRC_LIMITS = {7: (0, 64), 8: (1, 16), 9: (1, 16), 10: (3, 16)}      # sources an op of emap_plugin_chain_ex takes, by type

POLY_MAX_BATCH, POLY_MAX_VERTS, POLY_MAX_TILES = 4096, 256, 262144      # EMAP_POLY_MAX_BATCH / _MAX_VERTS / _MAX_TILES (caps)
POLY_MAP_LAYER, POLY_SEMANTIC, POLY_PLUGIN = 0, 1, 3      # EMAP_POLY_MAP_LAYER / _SEMANTIC / _PLUGIN: where the checker layer lies
POLY_HAS_NAN, POLY_POISON = 1, 2                    # EMAP_POLY_HAS_NAN / EMAP_POLY_POISON (verdict flags)

MODE = {"reference_fp16": 0, "fp32": 1}
PLANES = {"elevation": 0, "variance": 1, "is_valid": 2, "traversability": 3, "time": 4, "upper_bound": 5,
          "is_upper_bound": 6, "normal_x": 7, "normal_y": 8, "normal_z": 9, "traversability_input": 10}
STAGES = ["hist", "scan", "scatter", "gate", "fuse", "commit", "rays", "average", "overlap", "post"]

# every symbol include/emap_hip.h declares (checked by tests/test_abi.py without a GPU)
SYMBOLS = [
    "emap_abi_version", "emap_create", "emap_destroy", "emap_set_params", "emap_last_error", "emap_sync", "emap_clear",
    "emap_upload_points", "emap_upload_points_strip", "emap_strip_point_mask", "emap_declare_points_bucketed", "emap_set_points_device", "emap_set_points_device_split", "emap_bind_depth_image", "emap_bind_cloud_message", "emap_get_bound_points", "emap_point_index", "emap_update", "emap_count",
    "emap_set_drift_inputs", "emap_drift_sums_to_device", "emap_set_drift_inputs_device",
    "emap_local_drift_sums", "emap_set_scatter_mode", "emap_fuse", "emap_fuse_average", "emap_commit", "emap_rays", "emap_average", "emap_overlap_clear",
    "emap_dilate", "emap_traversability_normals", "emap_post", "emap_post_part", "emap_update_variance", "emap_update_time", "emap_get_stats",
    "emap_get_layer", "emap_set_layer", "emap_publish_layer", "emap_publish_grid_map", "emap_publish_grid_map_ex", "emap_publish_grid_windows", "emap_publish_point_cloud", "emap_plane_segmentation", "emap_planar_terrain", "emap_planar_regions", "emap_shift", "emap_strip_logical_begin", "emap_semantic_configure", "emap_semantic_update", "emap_frame_semantics",
    "emap_semantic_get_layer", "emap_semantic_set_layer", "emap_semantic_clear", "emap_semantic_get_alpha", "emap_semantic_set_alpha", "emap_semantic_class_max", "emap_semantic_accumulate", "emap_semantic_finalize", "emap_min_filter", "emap_max_filter", "emap_smooth_filter", "emap_erode", "emap_plugin_planes", "emap_plugin_plane_write", "emap_plugin_plane_read", "emap_plugin_chain", "emap_plugin_chain_ex", "emap_inpaint_u8", "emap_inpaint_telea_u8", "emap_inpaint_ns_u8", "emap_inpainter_create", "emap_inpainter_destroy", "emap_inpainter_set_steps", "emap_inpaint_telea_fronts_u8", "emap_image_correspondence", "emap_image_get_correspondence",
    "emap_image_fuse", "emap_image_set_tolerance", "emap_image_fuse_arrays", "emap_input_image_message", "emap_polygon_mask", "emap_polygon_safety", "emap_dilate_planes", "emap_halo_bytes", "emap_halo_pack", "emap_halo_unpack", "emap_normal_row_lag", "emap_normal_halo_pack", "emap_normal_halo_unpack", "emap_normal_lag_plan",
    "emap_comm_unique_id", "emap_comm_init", "emap_comm_destroy", "emap_comm_selftest", "emap_comm_count", "emap_comm_wire_bytes", "emap_comm_allreduce_host", "emap_comm_gather_layer", "emap_update_sharded", "emap_set_ray_mode",
    "emap_timer_begin", "emap_timer_end", "emap_enable_stage_timing", "emap_get_stage_times", "emap_last_update_path", "emap_small_frame_aborts", "emap_post_fused_launches",
]

_lib = None
ABI_VERSION = 3      # include/emap_hip.h: EMAP_ABI_VERSION (checked by load(), and across ranks by emap_comm_init)


class EmapError(RuntimeError):
    pass


def load():
    """Load the HIP library or raise (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EmapError(
            "libemap_hip.so is not built (%s). Run `python -m elevation_mapping_cupy_amd.csrc.build` "
            "(needs hipcc, target gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        lib = ct.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise EmapError("cannot load %s: %s (is the ROCm runtime installed?)" % (LIB_PATH, e)) from e
    lib.emap_last_error.restype = ct.c_char_p
    lib.emap_last_error.argtypes = [ct.c_void_p]
    for s in SYMBOLS:
        if s not in ("emap_last_error",):
            try:
                getattr(lib, s).restype = ct.c_int
            except AttributeError:
                if not os.environ.get("EMAP_HIP_LIB"):      # an older build handed in for an A/B run may lack newer entry points
                    raise
    if hasattr(lib, "emap_inpaint_telea_fronts_u8"):      # (pointer arguments: a handle must not be truncated to an int)
        u8p = ct.POINTER(ct.c_uint8)
        lib.emap_inpainter_create.argtypes = [ct.c_int32, ct.c_void_p, ct.POINTER(ct.c_void_p)]
        lib.emap_inpainter_destroy.argtypes = [ct.c_void_p]
        lib.emap_inpainter_set_steps.argtypes = [ct.c_void_p, ct.c_int32]
        lib.emap_inpaint_telea_fronts_u8.argtypes = [ct.c_void_p, u8p, u8p, ct.c_int32, ct.c_int32, ct.c_int32, u8p, ct.POINTER(ct.c_int32)]
    if hasattr(lib, "emap_bind_depth_image"):
        lib.emap_bind_depth_image.argtypes = [ct.c_void_p, ct.POINTER(EmapDepthDesc), ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_int64)]
        lib.emap_get_bound_points.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p]
    if hasattr(lib, "emap_bind_cloud_message"):
        lib.emap_bind_cloud_message.argtypes = [ct.c_void_p, ct.POINTER(EmapCloudMsgDesc), ct.c_void_p, ct.POINTER(ct.c_int64)]
    if hasattr(lib, "emap_input_image_message"):
        fp = ct.POINTER(ct.c_float)
        lib.emap_input_image_message.argtypes = [ct.c_void_p, ct.POINTER(EmapImageMsgDesc), ct.c_void_p, ct.c_float, ct.c_float, ct.c_float, fp, fp, fp, fp,
                                                 ct.POINTER(EmapImageSpec), ct.c_int32]
    if hasattr(lib, "emap_publish_grid_map"):
        lib.emap_publish_grid_map.argtypes = [ct.c_void_p, ct.POINTER(EmapGridLayer), ct.c_int32, ct.c_int32, ct.c_float, ct.c_int32, ct.POINTER(ct.c_float), ct.c_int64]
    if hasattr(lib, "emap_plugin_chain"):
        fp = ct.POINTER(ct.c_float)
        lib.emap_publish_grid_map_ex.argtypes = [ct.c_void_p, ct.POINTER(EmapGridLayerEx), ct.c_int32, ct.c_int32, ct.c_float, ct.c_int32, fp, ct.c_int64]
        lib.emap_plugin_planes.argtypes = [ct.c_void_p, ct.c_int32]
        lib.emap_plugin_plane_write.argtypes = [ct.c_void_p, ct.c_int32, fp]
        lib.emap_plugin_plane_read.argtypes = [ct.c_void_p, ct.c_int32, fp]
        lib.emap_plugin_chain.argtypes = [ct.c_void_p, ct.POINTER(EmapPluginOp), ct.c_int32, fp]
    if hasattr(lib, "emap_plugin_chain_ex"):
        lib.emap_plugin_chain_ex.argtypes = [ct.c_void_p, ct.POINTER(EmapPluginOp), ct.c_int32, ct.POINTER(ct.c_float), ct.POINTER(EmapPluginSrc), ct.c_int32]
    if hasattr(lib, "emap_polygon_safety"):
        lib.emap_polygon_safety.argtypes = [ct.c_void_p, ct.POINTER(ct.c_float), ct.POINTER(ct.c_int32), ct.c_int32, ct.c_float, ct.c_float, ct.c_int32, ct.c_int32,
                                            ct.c_float, ct.POINTER(EmapPolygonVerdict), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64)]
    if hasattr(lib, "emap_publish_grid_windows"):
        lib.emap_publish_grid_windows.argtypes = [ct.c_void_p, ct.POINTER(EmapGridLayerEx), ct.c_int32, ct.c_int32, ct.c_float, ct.c_int32,
                                                  ct.POINTER(EmapGridWindow), ct.c_int32, ct.POINTER(ct.c_float), ct.c_int64]
    if hasattr(lib, "emap_publish_point_cloud"):
        fp = ct.POINTER(ct.c_float)
        lib.emap_publish_point_cloud.argtypes = [ct.c_void_p, ct.POINTER(EmapCloudField), ct.c_int32, ct.c_float, ct.c_int32, fp, fp, ct.c_double, ct.c_int32,
                                                 ct.POINTER(ct.c_uint8), ct.c_int64, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int32)]
    if hasattr(lib, "emap_plane_segmentation"):
        lib.emap_plane_segmentation.argtypes = [ct.c_void_p, ct.POINTER(EmapGridLayerEx), ct.POINTER(EmapPlaneParams), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_float),
                                                ct.POINTER(EmapPlaneRecord), ct.c_int64, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64)]
    if hasattr(lib, "emap_planar_terrain"):
        lib.emap_planar_terrain.argtypes = [ct.c_void_p, ct.POINTER(EmapGridLayerEx), ct.POINTER(EmapPlaneParams), ct.POINTER(EmapTerrainParams), ct.POINTER(ct.c_int32),
                                            ct.POINTER(ct.c_float), ct.POINTER(EmapPlaneRecord), ct.c_int64, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64),
                                            ct.POINTER(EmapTerrainPlanes)]
    if hasattr(lib, "emap_planar_regions"):
        lib.emap_planar_regions.argtypes = [ct.c_void_p, ct.POINTER(ct.c_int32), ct.c_int32, ct.c_int32, ct.POINTER(EmapRegionParams), ct.POINTER(EmapRegionRing), ct.c_int64,
                                            ct.POINTER(ct.c_int32), ct.c_int64, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]
    got = int(lib.emap_abi_version())
    if got != ABI_VERSION and not os.environ.get("EMAP_HIP_LIB"):
        raise EmapError("%s speaks ABI version %d, this binding expects %d (include/emap_hip.h: EMAP_ABI_VERSION) -- rebuild with "
                        "`python -m elevation_mapping_cupy_amd.csrc.build`" % (LIB_PATH, got, ABI_VERSION))
    _lib = lib
    return lib


def fill_params(param, cell_n, mode):
    """Turn a ``Parameter`` dataclass into ``struct emap_params``."""
    P = EmapParams()
    P.cell_n = int(cell_n)
    P.mode = MODE[mode]
    for n in ("enable_edge_sharpen", "enable_visibility_cleanup", "enable_drift_compensation", "enable_overlap_clearance"):
        setattr(P, n, int(bool(getattr(param, n))))
    P.dilation_size = int(param.dilation_size)
    for n in _DOUBLES:
        if hasattr(param, n):
            setattr(P, n, float(getattr(param, n)))
    P.ray_step = float(param.resolution) / 2 ** 0.5  # reference custom_kernels.py:268
    for name in ("w1", "w2", "w3", "w_out"):
        arr = np.asarray(getattr(param, name), np.float32).ravel()
        getattr(P, name)[:] = arr.tolist()
    return P


def f32p(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_float))
