"""ctypes binding of liblidarslam_reg.so (include/lidarslam_reg.h).

The shared library is built in-tree by `__graft_entry__.build()` / `lidarslam_ros2_amd.build`.
There is no Python or CPU fallback: if the library is missing or no gfx950 device is visible,
the first compute call raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("LSR_LIB_NAME", "liblidarslam_reg.so"))

# enums (mirror include/lidarslam_reg.h)
OK = 0
POSE_GRAPH_MAX_VERTICES, POSE_GRAPH_MAX_BAND, POSE_GRAPH_MAX_OFFBAND_EDGES = 8192, 8, 64
POSE_GRAPH_LONG_MAX_OFFBAND_EDGES = 1024
METHOD_NDT, METHOD_GICP = 0, 1
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
(RESOLUTION, TRANSFORMATION_EPSILON, STEP_SIZE, OUTLIER_RATIO, MAX_CORRESPONDENCE_DISTANCE, ROTATION_EPSILON,
 EUCLIDEAN_FITNESS_EPSILON, GICP_EPSILON, MAP_ASSEMBLY_MS, POSE_GRAPH_BAND_SOLVE_MS, POSE_GRAPH_DENSE_MS,
 POSE_GRAPH_COMBINE_MS) = range(12)
PCD_FORMAT_MS, PCD_PIECE_RECORDS = 12, 50
PCD_PARSE_MS, PCD_READ_PIECE_BYTES, PCD_UNRESOLVED_TOKENS = 13, 52, 53
PCD_INFLATE_MS, PCD_READ_COMPRESSED = 14, 54
PCD_DEFLATE_MS = 15
(MAP_FILTER_BBOX_MS, MAP_FILTER_KEY_MS, MAP_FILTER_SORT_MS, MAP_FILTER_RUNS_MS, MAP_FILTER_CENTROID_MS,
 MAP_FILTER_WRITE_MS) = range(16, 22)
MAP_FILTER_KEY_BITS = 55
MAP_WINDOW_MS = 22
MAP_WINDOW_CELL_LIMIT = 1 << 24
POSE_SEARCH_MS = 23
POSE_SEARCH_MAX_POSES, POSE_SEARCH_MAX_KEPT = 1 << 20, 16
SCAN_CONTEXT_BUILD_MS, SCAN_CONTEXT_MATCH_MS = 24, 25
SCAN_CONTEXT_MAX_RINGS, SCAN_CONTEXT_MAX_SECTORS = 40, 120
DEPTH_IMAGES_MS, VISIBILITY_MS = 26, 27
VISIBILITY_PIECE_BYTES = 56
VISIBILITY_MAX_FACE_WIDTH, VISIBILITY_MAX_HEIGHT, VISIBILITY_MAX_NEIGHBOURS = 1024, 512, 64
PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED = 0, 1, 2           # lsr_pcd_data
PCD_DATA_KINDS = {"ascii": PCD_ASCII, "binary": PCD_BINARY, "binary_compressed": PCD_BINARY_COMPRESSED}
PCD_LZF_CHUNK_BYTES = 4096
PCD_READ_MAX_LINE_BYTES = 1024
ERR_NOT_IMPLEMENTED, ERR_INDEX_OVERFLOW = -6, -7
ERR_IO = -9
PCD_ASCII_MAX_LINE_BYTES, PCD_ASCII_MAX_HEADER_BYTES = 60, 256
NDT_REPLAY_MAX_ROWS, NDT_REPLAY_TRACE, DEBUG_MAX_COUNT = 512, 47, 1 << 20
DEBUG_SORT_MAX, DEBUG_LSD_PLAN_WORDS, DEBUG_CANARY_F32_BITS = 1 << 24, 11, 0x7FC0DEAD
(MAX_ITERATIONS, NEIGHBORHOOD, NUM_THREADS, K_CORRESPONDENCES, MAX_INNER_ITERATIONS, RANSAC_ITERATIONS,
 HESSIAN_D1_SIGN, PROFILE, NDT_WORKGROUP, NDT_TABLE_MODE, GRID_BUILDER, WAIT_MODE, NDT_QUAD, _UNASSIGNED_45, VOXEL_FILTER_FORM, NDT_SPLIT, TARGET_PREPARED,
 MAP_ASSEMBLY_FORM) = range(32, 50)
GICP_SOLVER = 51
GICP_GAUSS_NEWTON, GICP_BFGS = 0, 1

EXPORTED_SYMBOLS = [
    "lsr_version", "lsr_status_string", "lsr_last_error", "lsr_device_count", "lsr_create", "lsr_destroy",
    "lsr_set_f64", "lsr_set_i32", "lsr_get_f64", "lsr_get_i32", "lsr_set_input_target", "lsr_set_input_target_device",
    "lsr_set_input_target_frames", "lsr_set_input_source", "lsr_set_input_source_device", "lsr_set_input_source_filtered", "lsr_set_input_source_frontend", "lsr_voxel_grid_filter",
    "lsr_share_target", "lsr_wait_stream", "lsr_align", "lsr_align_batch",
    "lsr_get_final_transformation", "lsr_has_converged", "lsr_get_fitness_score", "lsr_search_loop", "lsr_ndt_grid_info",
    "lsr_ndt_grid_dump", "lsr_ndt_grid_centroids", "lsr_ndt_derivatives", "lsr_ndt_derivatives_pairs", "lsr_gicp_covariances", "lsr_nearest_neighbors", "lsr_get_profile",
    "lsr_debug_angle_tables", "lsr_debug_guess_pose", "lsr_debug_ndt_controller_replay", "lsr_debug_ndt_solve6", "lsr_debug_mt_math", "lsr_set_input_source_pc2", "lsr_get_source_pc2", "lsr_voxel_grid_filter_pc2", "lsr_shard_range", "lsr_comm_unique_id", "lsr_comm_create", "lsr_comm_destroy", "lsr_align_batch_sharded",
    "lsr_shard_plan", "lsr_align_batch_planned", "lsr_align_fitness_batch",
    "lsr_set_input_target_batch", "lsr_set_input_source_batch", "lsr_get_fitness_score_batch", "lsr_set_input_target_bcast", "lsr_get_source_pc2_device",
    "lsr_comm_all_gather_records", "lsr_set_input_target_frames_filtered", "lsr_prepare_target", "lsr_gicp_linearize",
    "lsr_imu_reset", "lsr_imu_push", "lsr_imu_receive", "lsr_imu_info", "lsr_deskew_pc2", "lsr_deskew_trace",
    "lsr_assemble_map", "lsr_pose_graph_edges", "lsr_optimize_pose_graph", "lsr_optimize_pose_graph_long",
    "lsr_format_pcd_ascii", "lsr_save_pcd_ascii", "lsr_save_map_pcd_ascii", "lsr_gicp_bfgs_trace",
    "lsr_sensor_transform_matrix", "lsr_transform_pc2", "lsr_set_input_source_pc2_tf", "lsr_odom_guess",
    "lsr_parse_pcd_header", "lsr_decode_pcd", "lsr_load_pcd", "lsr_set_input_target_pcd",
    "lsr_format_pcd", "lsr_save_pcd", "lsr_save_map_pcd", "lsr_lzf_deflate",
    "lsr_voxel_grid_filter_map", "lsr_assemble_map_filtered", "lsr_save_map_pcd_filtered",
    "lsr_map_window_around", "lsr_crop_map", "lsr_set_input_target_window",
    "lsr_ndt_score_poses", "lsr_pose_lattice_poses", "lsr_select_poses", "lsr_ndt_search_pose",
    "lsr_scan_context_tables", "lsr_scan_context_guess", "lsr_scan_context_build", "lsr_scan_context_match", "lsr_search_loop_appearance",
    "lsr_visibility_pairs", "lsr_depth_images_build", "lsr_visibility_votes", "lsr_assemble_map_static",
    "lsr_debug_lsd_plan", "lsr_debug_sort_pairs_u32", "lsr_debug_exclusive_scan_i32", "lsr_debug_sorted_runs",
]


class Result(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations", C.c_int32), ("score", C.c_double),
                ("n_evaluations", C.c_int32), ("n_correspondences", C.c_int32), ("gpu_ms", C.c_double)]


class Profile(C.Structure):
    _fields_ = [("deriv_ms_total", C.c_double), ("deriv_launches", C.c_int64), ("deriv_points", C.c_int64),
                ("deriv_pairs", C.c_int64)]


class SubMap(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("orientation", C.c_double * 4), ("distance", C.c_double),
                ("cloud", C.c_void_p), ("n_points", C.c_size_t)]


class LoopParams(C.Structure):
    _fields_ = [("threshold_loop_closure_score", C.c_double), ("distance_loop_closure", C.c_double),
                ("range_of_searching_loop_closure", C.c_double), ("search_submap_num", C.c_int),
                ("voxel_leaf_size", C.c_float), ("top_k", C.c_int), ("reserved", C.c_int)]


class LoopEdge(C.Structure):
    _fields_ = [("id_from", C.c_int), ("id_to", C.c_int), ("accepted", C.c_int), ("converged", C.c_int),
                ("iterations", C.c_int), ("n_target_points", C.c_int), ("candidate_distance", C.c_double),
                ("fitness_score", C.c_double), ("relative_pose", C.c_double * 16), ("final_transformation", C.c_float * 16)]


class PoseEdge(C.Structure):
    _fields_ = [("from_", C.c_int32), ("to", C.c_int32), ("measurement", C.c_double * 16)]


class PoseGraphParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("band", C.c_int32)]


class PoseGraphResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("chi2_before", C.c_double), ("chi2_after", C.c_double),
                ("lam", C.c_double), ("stop_reason", C.c_int32), ("reserved", C.c_int32), ("device_ms", C.c_double)]


class PoseGraphTrace(C.Structure):
    _fields_ = [("trials", C.c_int32), ("reserved", C.c_int32), ("chi2", C.c_double), ("lam", C.c_double), ("rho", C.c_double)]


class Pc2Layout(C.Structure):
    _fields_ = [("point_step", C.c_uint32), ("offset_x", C.c_uint32), ("offset_y", C.c_uint32), ("offset_z", C.c_uint32),
                ("offset_intensity", C.c_int32)]


class MapWindow(C.Structure):
    _fields_ = [("leaf", C.c_float), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


class PoseLattice(C.Structure):
    _fields_ = [("n", C.c_int32 * 3), ("step", C.c_double * 3), ("n_yaw", C.c_int32), ("yaw_step", C.c_double)]


class PoseSearchParams(C.Structure):
    _fields_ = [("lattice", PoseLattice), ("top_k", C.c_int32), ("min_sep_m", C.c_double), ("min_sep_rad", C.c_double)]


class PoseSearchReport(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("n_kept", C.c_int32), ("winner", C.c_int32), ("kept", C.c_int32 * 16),
                ("coarse_score", C.c_double * 16), ("refined16", C.c_float * 256), ("refined", Result * 16)]


class ScanContextParams(C.Structure):
    _fields_ = [("num_rings", C.c_int32), ("num_sectors", C.c_int32), ("max_radius", C.c_double), ("z_offset", C.c_double)]


class VisibilityParams(C.Structure):
    _fields_ = [("face_width", C.c_int32), ("height", C.c_int32), ("max_tan_elevation", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double), ("margin", C.c_double), ("keyframe_range", C.c_double), ("max_neighbours", C.c_int32),
                ("min_votes", C.c_int32), ("sensor_origin", C.c_double * 3)]


class AppearanceLoopParams(C.Structure):
    _fields_ = [("loop", LoopParams), ("sc", ScanContextParams), ("sc_distance_threshold", C.c_double), ("search", PoseSearchParams)]


class PcdInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("width", C.c_uint64), ("height", C.c_uint64), ("data_offset", C.c_uint64),
                ("point_step", C.c_uint32), ("data_kind", C.c_int32), ("has_intensity", C.c_int32), ("n_fields", C.c_int32),
                ("viewpoint", C.c_double * 7)]


class DeskewInfo(C.Structure):
    _fields_ = [("n_skipped", C.c_int32), ("start_missing", C.c_int32), ("half_index", C.c_int32), ("cursor", C.c_int32)]


class SensorTransform(C.Structure):
    _fields_ = [("translation", C.c_double * 3), ("rotation_xyzw", C.c_double * 4)]


class ShardRecord(C.Structure):
    _fields_ = [("T", C.c_float * 12), ("score", C.c_float), ("iterations", C.c_float), ("converged", C.c_float),
                ("fitness", C.c_float)]


class RegistrationError(RuntimeError):
    def __init__(self, status: int, where: str):
        lib = load()
        msg = lib.lsr_status_string(status).decode()
        detail = lib.lsr_last_error().decode()
        super().__init__(f"{where}: {msg} ({status}){': ' + detail if detail else ''}")
        self.status = status


_lib = None


def load() -> C.CDLL:
    """Load the HIP library; fail loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). lidarslam_ros2_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.lsr_version.restype = C.c_char_p
    L.lsr_status_string.restype = C.c_char_p
    L.lsr_status_string.argtypes = [C.c_int]
    L.lsr_last_error.restype = C.c_char_p
    L.lsr_device_count.argtypes = [ip]
    L.lsr_create.argtypes = [C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.lsr_destroy.argtypes = [vp]
    L.lsr_set_f64.argtypes = [vp, C.c_int, C.c_double]
    L.lsr_set_i32.argtypes = [vp, C.c_int, C.c_int]
    L.lsr_get_f64.argtypes = [vp, C.c_int, dp]
    L.lsr_get_i32.argtypes = [vp, C.c_int, ip]
    for name in ("lsr_set_input_target", "lsr_set_input_target_device", "lsr_set_input_source",
                 "lsr_set_input_source_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.lsr_share_target.argtypes = [vp, vp]
    L.lsr_wait_stream.argtypes = [vp, vp]
    L.lsr_set_input_target_frames.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, fp, C.c_int]
    L.lsr_set_input_target_frames_filtered.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, fp, C.c_int, C.c_float,
                                                       C.POINTER(C.c_size_t)]
    L.lsr_prepare_target.argtypes = [vp]
    L.lsr_set_input_source_filtered.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_set_input_source_frontend.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.c_float, C.c_int,
                                                C.POINTER(C.c_size_t)]
    L.lsr_voxel_grid_filter.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_float, vp, C.c_size_t, C.c_size_t,
                                        C.POINTER(C.c_size_t)]
    L.lsr_align.argtypes = [vp, fp, fp, C.POINTER(Result), vp, C.c_size_t]
    L.lsr_align_batch.argtypes = [C.POINTER(vp), C.c_int, fp, fp, C.POINTER(Result)]
    L.lsr_get_final_transformation.argtypes = [vp, fp]
    L.lsr_has_converged.argtypes = [vp, ip]
    L.lsr_get_fitness_score.argtypes = [vp, C.c_double, dp]
    L.lsr_get_fitness_score_batch.argtypes = [C.POINTER(vp), C.c_int, C.c_double, dp]
    L.lsr_set_input_target_batch.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_int]
    L.lsr_set_input_source_batch.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_int]
    L.lsr_search_loop.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.c_size_t, C.c_int, C.POINTER(LoopParams),
                                  C.POINTER(LoopEdge), C.c_int, ip]
    L.lsr_assemble_map.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, vp, C.c_size_t, C.POINTER(Pc2Layout),
                                   C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lsr_format_pcd_ascii.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_save_pcd_ascii.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_save_map_pcd_ascii.argtypes = [vp, C.c_char_p, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, C.POINTER(C.c_size_t)]
    L.lsr_format_pcd.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_save_pcd.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_save_map_pcd.argtypes = [vp, C.c_char_p, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_lzf_deflate.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_voxel_grid_filter_map.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.c_float, vp, C.c_size_t, C.POINTER(Pc2Layout),
                                            C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_assemble_map_filtered.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, C.c_float, vp, C.c_size_t,
                                            C.POINTER(Pc2Layout), C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_save_map_pcd_filtered.argtypes = [vp, C.c_char_p, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, C.c_float, C.c_int,
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lsr_map_window_around.argtypes = [dp, dp, C.c_float, C.POINTER(MapWindow)]
    L.lsr_crop_map.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(MapWindow), vp, C.c_size_t, C.POINTER(Pc2Layout),
                               C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_set_input_target_window.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(MapWindow), C.POINTER(C.c_size_t)]
    L.lsr_ndt_score_poses.argtypes = [vp, fp, C.c_size_t, dp, dp]
    L.lsr_pose_lattice_poses.argtypes = [fp, C.POINTER(PoseLattice), fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lsr_select_poses.argtypes = [dp, fp, C.c_size_t, C.c_int, C.c_double, C.c_double, ip, C.POINTER(C.c_int)]
    L.lsr_ndt_search_pose.argtypes = [vp, fp, C.POINTER(PoseSearchParams), fp, C.POINTER(Result), C.POINTER(PoseSearchReport)]
    L.lsr_scan_context_tables.argtypes = [C.POINTER(ScanContextParams), fp, fp]
    L.lsr_scan_context_guess.argtypes = [C.POINTER(SubMap), C.POINTER(SubMap), C.c_int, C.c_int, fp]
    L.lsr_scan_context_build.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, C.POINTER(ScanContextParams), vp, C.c_int]
    L.lsr_scan_context_match.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(ScanContextParams), fp, ip]
    L.lsr_search_loop_appearance.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.c_size_t, C.c_int, vp, C.c_int, C.c_int,
                                             C.POINTER(AppearanceLoopParams), C.POINTER(LoopEdge), ip, fp, C.c_int, ip]
    L.lsr_visibility_pairs.argtypes = [C.POINTER(SubMap), C.c_int, dp, C.POINTER(VisibilityParams), ip, ip, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lsr_depth_images_build.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, C.POINTER(VisibilityParams), C.c_int, vp,
                                         C.c_int]
    L.lsr_visibility_votes.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, vp, C.c_int,
                                       C.POINTER(VisibilityParams), vp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lsr_assemble_map_static.argtypes = [vp, C.POINTER(SubMap), C.c_int, C.POINTER(Pc2Layout), C.c_int, dp, vp, C.c_int,
                                          C.POINTER(VisibilityParams), vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lsr_parse_pcd_header.argtypes = [vp, C.c_size_t, C.POINTER(PcdInfo)]
    L.lsr_decode_pcd.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_load_pcd.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_set_input_target_pcd.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t)]
    L.lsr_pose_graph_edges.argtypes = [dp, C.c_int, C.c_int, C.POINTER(PoseEdge), C.c_size_t, C.POINTER(C.c_size_t)]
    for name in ("lsr_optimize_pose_graph", "lsr_optimize_pose_graph_long"):
        getattr(L, name).argtypes = [vp, dp, C.c_int, C.POINTER(PoseEdge), C.c_int, C.POINTER(PoseGraphParams), dp,
                                     C.POINTER(PoseGraphResult), C.POINTER(PoseGraphTrace)]
    L.lsr_ndt_grid_info.argtypes = [vp, ip]
    L.lsr_ndt_grid_dump.argtypes = [vp, ip, ip, dp, dp]
    L.lsr_ndt_grid_centroids.argtypes = [vp, fp]
    L.lsr_ndt_derivatives.argtypes = [vp, dp, fp, C.c_int, dp, dp, dp]
    L.lsr_ndt_derivatives_pairs.argtypes = [vp, dp, fp, C.c_int, dp, dp, dp, dp]
    L.lsr_gicp_covariances.argtypes = [vp, C.c_int, dp]
    L.lsr_nearest_neighbors.argtypes = [vp, fp, ip, fp]
    L.lsr_gicp_linearize.argtypes = [vp, fp, fp, C.c_int, fp, ip, ip, dp, fp, dp, fp, dp, ip, dp]
    L.lsr_gicp_bfgs_trace.argtypes = [vp, fp, fp, C.c_int32, dp, dp, dp, ip, ip, ip, ip, dp, ip]
    L.lsr_get_profile.argtypes = [vp, C.POINTER(Profile), C.c_int]
    L.lsr_debug_angle_tables.argtypes = [dp, C.c_int, fp, fp, fp, fp]
    L.lsr_debug_guess_pose.argtypes = [fp, dp]
    L.lsr_debug_ndt_controller_replay.argtypes = [vp, dp, C.c_double, C.c_double, C.c_int, C.c_int, dp, C.c_int, dp, C.POINTER(C.c_int)]
    L.lsr_debug_ndt_solve6.argtypes = [vp, dp, dp, C.c_int, dp]
    L.lsr_debug_mt_math.argtypes = [vp, dp, dp, C.c_int, dp, dp]
    up, cip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    L.lsr_debug_lsd_plan.argtypes = [C.c_size_t, C.c_int, cip]
    L.lsr_debug_sort_pairs_u32.argtypes = [vp, up, ip, C.c_size_t, C.c_int, C.c_int, up, ip, cip]
    L.lsr_debug_exclusive_scan_i32.argtypes = [vp, ip, C.c_size_t, C.c_int, C.c_int, ip]
    L.lsr_debug_sorted_runs.argtypes = [vp, up, ip, C.c_size_t, fp, fp, fp, fp, C.c_uint32, C.c_int, up, ip, fp, fp, fp, fp, cip, cip]
    L.lsr_set_input_source_pc2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_double, C.c_double, C.c_float, C.c_int,
                                           C.POINTER(C.c_size_t)]
    L.lsr_get_source_pc2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.POINTER(C.c_size_t)]
    L.lsr_get_source_pc2_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.POINTER(C.c_size_t)]
    L.lsr_voxel_grid_filter_pc2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_float, vp, C.c_size_t, C.POINTER(Pc2Layout),
                                            C.POINTER(C.c_size_t)]
    L.lsr_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
    L.lsr_shard_range.restype = None
    L.lsr_comm_unique_id.argtypes = [vp]
    L.lsr_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.lsr_comm_destroy.argtypes = [vp]
    L.lsr_align_batch_sharded.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, fp, C.c_int, C.POINTER(ShardRecord)]
    L.lsr_set_input_target_bcast.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int]
    L.lsr_align_fitness_batch.argtypes = [C.POINTER(vp), C.c_int, fp, fp, C.POINTER(Result), C.c_double, dp]
    i32p = C.POINTER(C.c_int32)
    L.lsr_shard_plan.argtypes = [C.c_int, dp, C.c_int, i32p, i32p, i32p]
    L.lsr_align_batch_planned.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, i32p, i32p, fp, C.c_int, C.POINTER(ShardRecord)]
    L.lsr_imu_reset.argtypes = [vp, C.c_double]
    L.lsr_imu_push.argtypes = [vp, fp, fp, fp, C.c_double]
    L.lsr_imu_receive.argtypes = [vp, dp, dp, dp, C.c_double]
    L.lsr_imu_info.argtypes = [vp, i32p]
    L.lsr_deskew_pc2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.c_double, C.c_int, vp, C.POINTER(DeskewInfo)]
    L.lsr_deskew_trace.argtypes = [vp, fp, i32p, C.POINTER(C.c_uint8)]
    L.lsr_sensor_transform_matrix.argtypes = [C.POINTER(SensorTransform), fp]
    L.lsr_transform_pc2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.POINTER(SensorTransform), C.c_int, vp]
    L.lsr_set_input_source_pc2_tf.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pc2Layout), C.POINTER(SensorTransform), C.c_double, C.c_double,
                                              C.c_float, C.c_int, C.POINTER(C.c_size_t)]
    L.lsr_odom_guess.argtypes = [fp, fp, fp, fp]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int or name not in ("lsr_version", "lsr_status_string", "lsr_last_error"):
            if name not in ("lsr_version", "lsr_status_string", "lsr_last_error", "lsr_shard_range"):
                fn.restype = C.c_int
    _lib = L
    return L


def check(status: int, where: str) -> None:
    if status != OK:
        raise RegistrationError(status, where)
