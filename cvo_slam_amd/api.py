"""ctypes binding of libcvo_hip.so, mirroring the reference's `cvo::cvo` interface
(thirdparty/cvo/include/cvo.hpp:216-276): same method names, argument meaning and
error behaviour, with the pcd_generator output (positions + features) handed in
where the reference takes the RGB / depth images.

Every call goes through the C ABI of include/cvo_hip.h.  There is no fallback: a
missing library raises at load time, a missing gfx950 device raises CvoError on the
first call.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CVO_OK, CVO_ERR_NOT_INITIALIZED, CVO_ERR_EMPTY_CLOUD, CVO_ERR_HIP, CVO_ERR_INVALID, CVO_ERR_NO_DEVICE, CVO_ERR_TIMEOUT, CVO_ERR_PADDING, CVO_ERR_RANK_FAILED = range(9)
SLOT_FIXED, SLOT_MOVING, SLOT_PREVIOUS = 0, 1, 2
RESULT_FLOATS = 16
# arithmetic modes (cvo_hip.h: CVO_ARITH_*; the same bits as the test oracle's reference-noise variants)
ARITH_BASE, ARITH_F32_ROOTS, ARITH_F32_LOGM, ARITH_ROW_LAZY16 = 0, 2, 4, 8
ARITH_EIGEN337 = ARITH_F32_ROOTS | ARITH_F32_LOGM | ARITH_ROW_LAZY16
ARITH_NAMES = {"base": ARITH_BASE, "eigen337": ARITH_EIGEN337}


def arith_flags(mode) -> int:
    """An arithmetic mode as its CVO_ARITH_* bits: an int, or one of the names in ARITH_NAMES."""
    if isinstance(mode, str):
        if mode not in ARITH_NAMES:
            raise ValueError(f"unknown arithmetic mode {mode!r} (known: {', '.join(ARITH_NAMES)})")
        return ARITH_NAMES[mode]
    return int(mode)


class CvoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libcvo_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("ell", C.c_float), ("sigma", C.c_float), ("sp_thres", C.c_float), ("c", C.c_float), ("d", C.c_float),
                ("c_ell", C.c_float), ("c_sigma", C.c_float), ("max_iter", C.c_int), ("min_step", C.c_float),
                ("eps", C.c_float), ("eps_2", C.c_float)]


class InnP(C.Structure):
    _fields_ = [("value", C.c_float), ("num", C.c_int), ("num_e", C.c_int)]


class TraceRow(C.Structure):
    _fields_ = [("omega", C.c_float * 3), ("v", C.c_float * 3), ("nnz", C.c_int), ("candidates", C.c_int),
                ("B", C.c_double), ("C", C.c_double), ("D", C.c_double), ("E", C.c_double),
                ("step", C.c_float), ("ell", C.c_float), ("dist", C.c_float), ("pad_", C.c_int)]


class PairResult(C.Structure):
    _fields_ = [("transform", C.c_float * 12), ("R", C.c_float * 9), ("T", C.c_float * 3), ("ell", C.c_float),
                ("iter", C.c_int), ("A_nonzero", C.c_int), ("iterations_run", C.c_int), ("status", C.c_int),
                ("rebuilds", C.c_int), ("dense_fallbacks", C.c_int)]


class Camera(C.Structure):
    """cvo::camera_info (data_type.h:33-39)."""
    _fields_ = [("scaling_factor", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class DeviceImage(C.Structure):         # cvo_device_image: a frame in caller-owned device memory
    _fields_ = [("bgr8", C.c_void_p), ("depth16", C.c_void_p), ("bgr_pitch", C.c_longlong), ("depth_pitch", C.c_longlong),
                ("pixel_bytes", C.c_int), ("swap_rb", C.c_int)]


class DeviceCloud(C.Structure):         # cvo_device_cloud: a point cloud in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("xyz_stride", C.c_longlong), ("feat_point_stride", C.c_longlong),
                ("feat_channel_stride", C.c_longlong), ("n", C.c_int), ("pad_", C.c_int)]


class ReduceParams(C.Structure):         # cvo_reduce_params: one voxel-grid filter for all clouds of a call
    _fields_ = [("voxel", C.c_float), ("mode", C.c_int), ("min_points", C.c_int), ("pad_", C.c_int)]


class ReducedCloud(C.Structure):         # cvo_reduced_cloud: one cloud's output arrays in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("count", C.c_void_p), ("source", C.c_void_p), ("map", C.c_void_p),
                ("cap", C.c_int), ("pad_", C.c_int)]


class FuseMember(C.Structure):           # cvo_fuse_member: one posed cloud of a group (pose: row-major 3 x 4, host memory)
    _fields_ = [("cloud", DeviceCloud), ("pose", C.c_float * 12)]


class FuseParams(C.Structure):           # cvo_fuse_params: one filter for all groups of a call
    _fields_ = [("voxel", C.c_float), ("mode", C.c_int), ("min_points", C.c_int), ("min_views", C.c_int)]


class FusedCloud(C.Structure):           # cvo_fused_cloud: one group's output arrays in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("count", C.c_void_p), ("source", C.c_void_p), ("map", C.c_void_p),
                ("views", C.c_void_p), ("view_mask", C.c_void_p), ("cap", C.c_int), ("pad_", C.c_int)]


class FrameCloud(C.Structure):           # cvo_frame_cloud: one frame's dense cloud in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p)]


class FuseFrame(C.Structure):            # cvo_fuse_frame: one posed frame of a group (pose: row-major 3 x 4, host memory; cam: index into the call's cameras)
    _fields_ = [("image", DeviceImage), ("pose", C.c_float * 12), ("cam", C.c_int), ("pad_", C.c_int)]


class View(C.Structure):                 # cvo_view: one posed cloud seen by one camera (pose: row-major 3 x 4, host memory; cam: index into the call's cameras)
    _fields_ = [("cloud", DeviceCloud), ("pose", C.c_float * 12), ("cam", C.c_int), ("pad_", C.c_int)]


class ViewParams(C.Structure):           # cvo_view_params: one image grid, mode and depth range for all views of a call
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("cell", C.c_int), ("mode", C.c_int),
                ("z_near", C.c_float), ("z_far", C.c_float), ("slack", C.c_float), ("depth_tol", C.c_float)]


class ViewedCloud(C.Structure):          # cvo_viewed_cloud: one view's output arrays in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("source", C.c_void_p), ("pixel", C.c_void_p), ("relation", C.c_void_p),
                ("map", C.c_void_p), ("depth", C.c_void_p), ("index", C.c_void_p), ("cap", C.c_int), ("pad_", C.c_int)]


class MapFilter(C.Structure):            # cvo_map_filter: which rows of one resident map an extract keeps
    _fields_ = [("min_points", C.c_int), ("min_views", C.c_int), ("min_last_stamp", C.c_int), ("pad_", C.c_int)]


class MapKeep(C.Structure):              # cvo_map_keep: which rows of one resident map survive a compaction
    _fields_ = [("min_last_stamp", C.c_int), ("min_views", C.c_int), ("probation_from", C.c_int), ("pad_", C.c_int)]


class MapCloud(C.Structure):             # cvo_map_cloud: one map's extracted arrays in caller-owned device memory
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("count", C.c_void_p), ("views", C.c_void_p), ("view_mask", C.c_void_p),
                ("last_stamp", C.c_void_p), ("born", C.c_void_p), ("row", C.c_void_p), ("cap", C.c_int), ("pad_", C.c_int)]


class MapView(C.Structure):              # cvo_map_view: one resident map seen by one camera under one filter (pose: row-major 3 x 4, host memory)
    _fields_ = [("map", C.c_int), ("cam", C.c_int), ("filter", MapFilter), ("pose", C.c_float * 12)]


class MapProbe(C.Structure):             # cvo_map_probe: which resident map one posed member is looked up in, how far around each point, under which filter
    _fields_ = [("map", C.c_int), ("reach", C.c_int), ("filter", MapFilter)]


class ProbedPoints(C.Structure):         # cvo_probed_points: one probe's output arrays in caller-owned device memory
    _fields_ = [("row", C.c_void_p), ("dist2", C.c_void_p), ("count", C.c_void_p), ("views", C.c_void_p), ("last_stamp", C.c_void_p), ("hit", C.c_void_p)]


class MapSnapshot(C.Structure):          # cvo_map_snapshot: one map's rows as six caller-owned device arrays; rows: the capacity (snapshot) or the rows to put in (restore)
    _fields_ = [("keys", C.c_void_p), ("sums", C.c_void_p), ("count", C.c_void_p), ("view_mask", C.c_void_p), ("last_stamp", C.c_void_p),
                ("born", C.c_void_p), ("rows", C.c_int), ("pad_", C.c_int)]


class MapMerge(C.Structure):             # cvo_map_merge: one source map added into one destination map; all_rows: every row, else those `filter` keeps
    _fields_ = [("dst_map", C.c_int), ("src_map", C.c_int), ("all_rows", C.c_int), ("pad_", C.c_int), ("filter", MapFilter)]


class LcScores(C.Structure):
    _fields_ = [("inn_prior", InnP), ("inn_lc_prior", InnP), ("inn_pre", InnP), ("inn_post", InnP), ("inn_fixed_pcd", InnP),
                ("inn_moving_pcd", InnP), ("post_hessian", C.c_double * 36), ("inliers_svd", C.c_int), ("inliers_pnpransac", C.c_int),
                ("cos_angle", C.c_float), ("accept", C.c_int)]


class AdaptiveParams(C.Structure):      # cvo_adaptive_params (adaptive_cvo.cpp:27-46)
    _fields_ = [("ell_init", C.c_float), ("ell_min", C.c_float), ("ell_max", C.c_float), ("dl_step", C.c_float), ("sigma", C.c_float),
                ("sp_thres", C.c_float), ("c", C.c_float), ("d", C.c_float), ("c_ell", C.c_float), ("c_sigma", C.c_float),
                ("max_iter", C.c_int), ("min_step", C.c_float), ("eps", C.c_float), ("eps_2", C.c_float)]


class AdaptiveRow(C.Structure):
    _fields_ = [("omega", C.c_float * 3), ("v", C.c_float * 3), ("dl", C.c_float), ("ell", C.c_float), ("step", C.c_float),
                ("nnz_xy", C.c_int), ("nnz_xx", C.c_int), ("nnz_yy", C.c_int)]


class TrackScores(C.Structure):
    _fields_ = [("inn_pre", InnP), ("inn_post", InnP), ("inn_fixed_pcd", InnP), ("inn_moving_pcd", InnP), ("post_hessian", C.c_double * 36),
                ("inliers", C.c_int), ("cos_angle", C.c_float)]


class PointSupportDst(C.Structure):      # cvo_point_support_dst: one pair's four output arrays (host or device memory, by entry point)
    _fields_ = [("sum_moving", C.c_void_p), ("count_moving", C.c_void_p), ("sum_fixed", C.c_void_p), ("count_fixed", C.c_void_p)]


class MatchFit(C.Structure):             # cvo_match_fit: one direction's fit record of a point-matches call
    _fields_ = [("rows", C.c_int), ("matched", C.c_int), ("sum_w", C.c_double), ("sum_w_res2", C.c_double)]


class PointMatchesDst(C.Structure):      # cvo_point_matches_dst: one pair's ten output arrays and its two fit records (host or device memory, by entry point)
    _fields_ = [("best_moving", C.c_void_p), ("best_value_moving", C.c_void_p), ("mean_moving", C.c_void_p), ("sum_moving", C.c_void_p), ("count_moving", C.c_void_p),
                ("best_fixed", C.c_void_p), ("best_value_fixed", C.c_void_p), ("mean_fixed", C.c_void_p), ("sum_fixed", C.c_void_p), ("count_fixed", C.c_void_p),
                ("fit", C.c_void_p)]


class PoseModel(C.Structure):            # cvo_pose_model: value, se(3) gradient and Hessian of the inner product at one pose
    _fields_ = [("value", C.c_float), ("num", C.c_int), ("grad", C.c_double * 6), ("hess", C.c_double * 36)]


class TrackStep(C.Structure):
    """cvo_track_step: one stream's share of a tracker step (cvo_hip.h: cvo_tracks_wait)."""
    _fields_ = [("phase", C.c_int), ("points", C.c_int), ("odometry", PairResult), ("odometry_scores", TrackScores),
                ("keyframe", PairResult), ("keyframe_scores", TrackScores), ("initial_guess", C.c_float * 12)]


# every symbol include/cvo_hip.h declares (tests check the .so exports exactly these)
ABI_SYMBOLS = [
    "cvo_last_error", "cvo_device_count", "cvo_default_params", "cvo_create", "cvo_destroy", "cvo_set_pcd", "cvo_align",
    "cvo_align_traced", "cvo_match_odometry", "cvo_match_keyframe", "cvo_function_inner_product", "cvo_se3_hessian",
    "cvo_compute_innerproduct", "cvo_compute_innerproduct_lc", "cvo_update_fixed_pcd", "cvo_update_previous_pcd",
    "cvo_reset_keyframe", "cvo_reset_transform", "cvo_reset_initial", "cvo_get_fixed_and_moving_number",
    "cvo_get_iteration_number", "cvo_get_A_nonzero", "cvo_get_transform", "cvo_get_prev_accum_transform", "cvo_get_init",
    "cvo_get_first_frame", "cvo_set_first_frame", "cvo_get_state", "cvo_set_state", "cvo_set_workgroups",
    "cvo_batch_create", "cvo_batch_destroy", "cvo_batch_set_pair", "cvo_batch_set_state", "cvo_batch_set_workgroups",
    "cvo_batch_reset_states", "cvo_batch_align_async", "cvo_batch_wait", "cvo_batch_last_launch",
    "cvo_batch_results_to_device", "cvo_batch_last_phase_seconds", "cvo_batch_compute_innerproduct_lc",
    "cvo_set_pcd_images", "cvo_shared_cloud_count", "cvo_stage_next_frame", "cvo_staged_frame_count", "cvo_queued_score_count", "cvo_set_num_want", "cvo_match_odometry_images", "cvo_match_keyframe_images", "cvo_get_cloud", "cvo_get_selected_points",
    "cvo_batch_enqueue_innerproduct", "cvo_batch_innerproduct_results", "cvo_batch_compute_innerproduct",
    "cvo_selftest_cubic_step", "cvo_selftest_exp_sek3", "cvo_selftest_dist_se3", "cvo_selftest_libm", "cvo_selftest_pair_values",
    "cvo_function_inner_product_clouds", "cvo_se3_hessian_clouds", "cvo_batch_set_max_workgroups", "cvo_batch_set_adoption", "cvo_batch_last_adoptions", "cvo_batch_last_adoption_retractions", "cvo_batch_last_launch_shape", "cvo_batch_queue_class",
    "cvo_adaptive_default_params", "cvo_adaptive_align",
    "cvo_shard_range", "cvo_comm_unique_id", "cvo_comm_create", "cvo_comm_create_all", "cvo_host_register", "cvo_host_unregister", "cvo_comm_destroy", "cvo_comm_info", "cvo_comm_set_gather_stream", "cvo_comm_library_path", "cvo_batch_gather_results",
    "cvo_gather_results", "cvo_multi_create", "cvo_multi_destroy", "cvo_multi_batch", "cvo_multi_align_async", "cvo_multi_wait",
    "cvo_batch_set_pairs", "cvo_batch_result_records", "cvo_shard_block", "cvo_batch_gather_results_padded", "cvo_batch_padded_records",
    "cvo_compact_records", "cvo_gather_results_padded", "cvo_multi_align_async_v", "cvo_batch_done", "cvo_batch_set_tail_scores", "cvo_batch_last_tail_answers", "cvo_batch_last_pair_seconds", "cvo_batch_last_pair_spans", "cvo_batch_last_tail_seconds", "cvo_set_tail_scores", "cvo_batch_last_cull_masks", "cvo_batch_last_nonzeros",
    "cvo_set_arith_mode", "cvo_get_arith_mode", "cvo_batch_set_arith_mode", "cvo_batch_get_arith_mode",
    "cvo_selftest_cubic_step_f32eig", "cvo_selftest_dist_se3_f32logm",
    "cvo_batch_set_pairs_images", "cvo_batch_set_num_want", "cvo_batch_get_cloud", "cvo_batch_get_selected_points",
    "cvo_batch_advance_images", "cvo_batch_reset_stream", "cvo_batch_align_pairs_async", "cvo_batch_get_prev_accum_transform",
    "cvo_selftest_reset_initial", "cvo_tracks_create", "cvo_tracks_destroy", "cvo_tracks_set_num_want", "cvo_tracks_set_arith_mode", "cvo_tracks_reset",
    "cvo_tracks_step_async", "cvo_tracks_done", "cvo_tracks_wait", "cvo_tracks_commit", "cvo_tracks_get_cloud", "cvo_tracks_get_selected_points",
    "cvo_tracks_get_state",
    "cvo_batch_stage_images", "cvo_batch_advance_staged", "cvo_batch_staged_count",
    "cvo_tracks_stage_async", "cvo_tracks_step_staged_async", "cvo_tracks_staged_count",
    "cvo_check_device_images", "cvo_selftest_ingest_images", "cvo_batch_set_pairs_device_images", "cvo_batch_advance_device_images",
    "cvo_batch_stage_device_images", "cvo_tracks_step_device_async", "cvo_tracks_stage_device_async",
    "cvo_check_device_clouds", "cvo_selftest_ingest_clouds", "cvo_batch_set_pairs_device_clouds", "cvo_batch_advance_device_clouds",
    "cvo_tracks_step_device_clouds_async",
    "cvo_point_support", "cvo_batch_point_support", "cvo_batch_point_support_device", "cvo_tracks_point_support", "cvo_tracks_point_support_device",
    "cvo_point_matches", "cvo_batch_point_matches", "cvo_batch_point_matches_device", "cvo_tracks_point_matches", "cvo_tracks_point_matches_device",
    "cvo_score_hypotheses", "cvo_batch_score_hypotheses", "cvo_batch_seed_hypotheses_async", "cvo_batch_hypothesis_results",
    "cvo_pose_models", "cvo_batch_pose_models", "cvo_batch_result_models",
    "cvo_reducer_create", "cvo_reducer_destroy", "cvo_reducer_info", "cvo_check_reduce_clouds", "cvo_reduce_device_clouds", "cvo_count_voxels",
    "cvo_check_fuse_clouds", "cvo_fuse_device_clouds",
    "cvo_check_device_frames", "cvo_frames_to_device_clouds", "cvo_reduce_device_frames", "cvo_count_frame_voxels", "cvo_check_fuse_frames",
    "cvo_fuse_device_frames",
    "cvo_check_view_clouds", "cvo_view_device_clouds",
    "cvo_maps_create", "cvo_maps_destroy", "cvo_maps_info", "cvo_maps_clear", "cvo_maps_rows", "cvo_check_maps_integrate_clouds",
    "cvo_check_maps_integrate_frames", "cvo_maps_integrate_clouds", "cvo_maps_integrate_frames", "cvo_check_maps_extract", "cvo_maps_extract",
    "cvo_check_maps_compact", "cvo_maps_compact", "cvo_check_maps_view", "cvo_maps_view",
    "cvo_check_maps_probe_clouds", "cvo_maps_probe_clouds", "cvo_check_maps_probe_frames", "cvo_maps_probe_frames",
    "cvo_check_maps_snapshot", "cvo_maps_snapshot", "cvo_check_maps_restore", "cvo_maps_restore",
    "cvo_check_maps_merge", "cvo_maps_merge",
    "cvo_selftest_voxel_slots",
]
MAX_HYPOTHESES = 64                      # CVO_MAX_HYPOTHESES
REDUCE_MEAN, REDUCE_CENTRAL = 0, 1       # CVO_REDUCE_MEAN, CVO_REDUCE_CENTRAL
REDUCE_MODES = {"mean": REDUCE_MEAN, "central": REDUCE_CENTRAL}
REDUCE_MAX_POINTS = 1048575              # CVO_REDUCE_MAX_POINTS
REDUCE_MAX_VOXELS = 16                   # CVO_REDUCE_MAX_VOXELS
FUSE_MAX_MEMBERS = 64                    # members of a group: the bits of a view mask
FUSE_WANT = ("count", "source", "map", "views", "view_mask")
FRAME_MAX_STEP = 16                      # a frame's sub-grid step: 1 .. 16
VIEW_FRONT, VIEW_SURFACE = 0, 1          # CVO_VIEW_FRONT, CVO_VIEW_SURFACE
VIEW_MODES = {"front": VIEW_FRONT, "surface": VIEW_SURFACE}
VIEW_WANT = ("source", "pixel", "relation", "map", "depth", "index")
VIEW_MAX_CELL = 16                       # a z-cell's side in pixels: 1 .. 16
VIEW_MAX_SIZE = 8192                     # the most pixels along either side of a view's image
MAP_MAX_ROWS = 1048575                   # CVO_MAP_MAX_ROWS
MAP_MAX_COUNT = 16777215                 # CVO_MAP_MAX_COUNT
MAP_INTEGRATE, MAP_REMOVE, MAP_REMOVE_PRESENT = 1, -1, -2      # CVO_MAP_*: the sign of an update
MAP_WANT = ("count", "views", "view_mask", "last_stamp", "born", "row")
PROBE_WANT = ("dist2", "count", "views", "last_stamp")      # what a probe returns beside row, one entry per point
PROBE_ABSENT, PROBE_INVALID, PROBE_FILTERED = -1, -3, -4     # a probed point's row when it has none
SNAPSHOT_FIELDS = (("keys", 8, "iu", ()), ("sums", 8, "i", (8,)), ("count", 4, "iu", ()), ("view_mask", 8, "iu", ()), ("last_stamp", 4, "i", ()),
                   ("born", 4, "i", ()))    # a snapshot's arrays: name, item bytes, integer kinds that carry it, a row's shape
MAP_MERGE_MAX_LEVEL = 4                  # CVO_MAP_MERGE_MAX_LEVEL: a merge's destination voxel is the source's times 2^0 .. 2^4
RESTORE_BAD_KEY, RESTORE_BAD_COUNT, RESTORE_BAD_STAMP, RESTORE_BAD_SUM, RESTORE_DUPLICATE = 1, 2, 4, 8, 16   # a refused restore's bits

_lib = None


def lib_path() -> str:
    # CVO_HIP_LIB: experiment builds of the same ABI (scripts/gpu_*.sh); products leave it unset
    return os.environ.get("CVO_HIP_LIB") or os.path.join(HERE, "libcvo_hip.so")


def load_library():
    """Load libcvo_hip.so (built in-tree by cvo_slam_amd/build.py).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: build it with `python -m cvo_slam_amd.build` (hipcc, gfx950). "
                                "There is no CPU fallback.")
    L = C.CDLL(path)
    if os.environ.get("CVO_HIP_LIB"):
        # an experiment build or an OLDER build of the ABI (regression checks against last round's library): entry points it lacks are bound to
        # a stand-in that fails when called.  The product library (no CVO_HIP_LIB) must export everything: tests/test_capi_symbols.py.
        class _Missing:
            def __init__(self, name): self.name = name; self.argtypes = None; self.restype = None
            def __call__(self, *a): raise CvoError(4, f"{self.name} is not exported by {path}")
        class _Tolerant(C.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("cvo_"): raise
                    m = _Missing(name); self.__dict__[name] = m; return m
        L = _Tolerant(path)
    fp = C.POINTER(C.c_float); dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int); vp = C.c_void_p
    L.cvo_last_error.restype = C.c_char_p
    L.cvo_default_params.argtypes = [C.POINTER(Params)]
    L.cvo_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(vp)]
    L.cvo_destroy.argtypes = [vp]
    L.cvo_set_pcd.argtypes = [vp, fp, fp, C.c_int]
    L.cvo_align.argtypes = [vp]
    L.cvo_align_traced.argtypes = [vp, C.POINTER(TraceRow), C.c_int, ip]
    L.cvo_match_odometry.argtypes = [vp, fp, fp, C.c_int, dp]
    L.cvo_match_keyframe.argtypes = [vp, fp, fp, C.c_int, dp]
    L.cvo_function_inner_product.argtypes = [vp, C.c_int, fp, C.c_int, C.POINTER(InnP)]
    L.cvo_se3_hessian.argtypes = [vp, C.c_int, fp, C.c_int, dp, ip]
    L.cvo_compute_innerproduct.argtypes = [vp, C.POINTER(InnP), C.POINTER(InnP), dp, fp, ip, C.POINTER(InnP), C.POINTER(InnP), fp]
    L.cvo_compute_innerproduct_lc.argtypes = [vp] + [C.POINTER(InnP)] * 4 + [dp, fp, fp, fp, fp, ip, ip, C.POINTER(InnP), C.POINTER(InnP), fp]
    L.cvo_update_fixed_pcd.argtypes = [vp]
    L.cvo_update_previous_pcd.argtypes = [vp]
    L.cvo_reset_keyframe.argtypes = [vp, fp]
    L.cvo_reset_transform.argtypes = [vp, fp]
    L.cvo_reset_initial.argtypes = [vp, fp, fp]
    L.cvo_get_fixed_and_moving_number.argtypes = [vp, ip, ip]
    L.cvo_get_iteration_number.argtypes = [vp, ip]
    L.cvo_get_A_nonzero.argtypes = [vp, ip]
    L.cvo_get_transform.argtypes = [vp, fp]
    L.cvo_get_prev_accum_transform.argtypes = [vp, fp, fp]
    L.cvo_get_init.argtypes = [vp, ip]
    L.cvo_get_first_frame.argtypes = [vp, ip]
    L.cvo_set_first_frame.argtypes = [vp, C.c_int]
    L.cvo_get_state.argtypes = [vp, fp, fp, fp]
    L.cvo_set_state.argtypes = [vp, fp, fp, C.c_float]
    L.cvo_set_workgroups.argtypes = [vp, C.c_int]
    L.cvo_batch_create.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_batch_destroy.argtypes = [vp]
    L.cvo_batch_set_pair.argtypes = [vp, C.c_int, fp, fp, C.c_int, fp, fp, C.c_int]
    L.cvo_batch_set_state.argtypes = [vp, C.c_int, fp, fp, C.c_float]
    L.cvo_batch_set_workgroups.argtypes = [vp, C.c_int]
    L.cvo_batch_reset_states.argtypes = [vp]
    L.cvo_batch_align_async.argtypes = [vp, C.c_int, vp]
    L.cvo_batch_wait.argtypes = [vp, C.POINTER(PairResult), C.c_int]
    L.cvo_batch_last_launch.argtypes = [vp, fp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.cvo_batch_results_to_device.argtypes = [vp, vp, C.c_int, vp]
    L.cvo_batch_last_phase_seconds.argtypes = [vp, dp]
    L.cvo_batch_compute_innerproduct_lc.argtypes = [vp, C.c_int, fp, fp, fp, C.POINTER(LcScores)]
    L.cvo_set_pcd_images.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(Camera)]
    L.cvo_set_num_want.argtypes = [vp, C.c_int]
    L.cvo_shared_cloud_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_stage_next_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(Camera)]
    L.cvo_staged_frame_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_queued_score_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_match_odometry_images.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(Camera), dp]
    L.cvo_match_keyframe_images.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(Camera), dp]
    L.cvo_get_cloud.argtypes = [vp, C.c_int, fp, fp, C.c_int, ip]
    L.cvo_get_selected_points.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    L.cvo_batch_set_pairs_images.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Camera), ip, ip, ip]
    L.cvo_batch_set_num_want.argtypes = [vp, C.c_int]
    L.cvo_batch_advance_images.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Camera), ip, ip]
    L.cvo_batch_reset_stream.argtypes = [vp, C.c_int]
    L.cvo_batch_align_pairs_async.argtypes = [vp, C.c_int, ip, vp]
    L.cvo_batch_get_prev_accum_transform.argtypes = [vp, C.c_int, fp, fp]
    L.cvo_batch_get_cloud.argtypes = [vp, C.c_int, C.c_int, fp, fp, C.c_int, ip]
    L.cvo_batch_get_selected_points.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, ip]
    L.cvo_batch_enqueue_innerproduct.argtypes = [vp, C.c_int]
    L.cvo_batch_innerproduct_results.argtypes = [vp, C.c_int, C.POINTER(TrackScores)]
    L.cvo_batch_compute_innerproduct.argtypes = [vp, C.c_int, C.POINTER(TrackScores)]
    for name in ("cvo_selftest_cubic_step", "cvo_selftest_exp_sek3", "cvo_selftest_dist_se3", "cvo_selftest_libm", "cvo_selftest_cubic_step_f32eig",
                 "cvo_selftest_dist_se3_f32logm", "cvo_selftest_reset_initial"):
        getattr(L, name).argtypes = [C.c_int, C.c_int, fp, fp]
    L.cvo_selftest_pair_values.argtypes = [C.c_int, C.POINTER(Params), C.c_float, C.c_int, fp, fp, fp]
    L.cvo_selftest_voxel_slots.argtypes = [C.c_int, C.c_int, fp, C.c_float, C.c_uint, ip, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]
    L.cvo_function_inner_product_clouds.argtypes = [vp, fp, fp, C.c_int, fp, fp, C.c_int, C.POINTER(InnP)]
    L.cvo_se3_hessian_clouds.argtypes = [vp, fp, fp, C.c_int, fp, fp, C.c_int, dp, ip]
    L.cvo_batch_set_max_workgroups.argtypes = [vp, C.c_int]
    L.cvo_batch_set_adoption.argtypes = [vp, C.c_int]
    for name in ("cvo_set_arith_mode", "cvo_batch_set_arith_mode"):
        getattr(L, name).argtypes = [vp, C.c_int]
    for name in ("cvo_get_arith_mode", "cvo_batch_get_arith_mode"):
        getattr(L, name).argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_batch_last_adoptions.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_batch_last_adoption_retractions.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_batch_last_launch_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_batch_queue_class.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_adaptive_default_params.argtypes = [C.POINTER(AdaptiveParams)]
    L.cvo_adaptive_align.argtypes = [C.c_int, C.POINTER(AdaptiveParams), fp, fp, C.c_int, fp, fp, C.c_int, fp, fp, fp, fp, ip, C.POINTER(AdaptiveRow), C.c_int, ip]
    L.cvo_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
    L.cvo_comm_unique_id.argtypes = [C.c_char_p]
    L.cvo_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_comm_create_all.argtypes = [ip, C.c_int, C.POINTER(vp)]
    L.cvo_comm_destroy.argtypes = [vp]
    L.cvo_comm_info.argtypes = [vp, ip, ip]
    L.cvo_host_register.argtypes = [vp, C.c_size_t]
    L.cvo_host_unregister.argtypes = [vp]
    L.cvo_comm_set_gather_stream.argtypes = [vp, C.c_int]
    L.cvo_comm_library_path.argtypes = [C.c_char_p, C.c_int]
    L.cvo_batch_gather_results.argtypes = [vp, vp, C.c_int, vp]
    L.cvo_gather_results.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_multi_create.argtypes = [C.POINTER(Params), ip, C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_multi_destroy.argtypes = [vp]
    L.cvo_multi_batch.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.cvo_multi_align_async.argtypes = [vp, C.c_int]
    L.cvo_multi_wait.argtypes = [vp, C.c_int, fp]
    pp = C.POINTER(fp)
    L.cvo_batch_set_pairs.argtypes = [vp, C.c_int, C.c_int, pp, pp, ip, pp, pp, ip]
    L.cvo_batch_result_records.argtypes = [vp, C.POINTER(vp)]
    L.cvo_shard_block.argtypes = [C.c_int, C.c_int]
    L.cvo_batch_gather_results_padded.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.cvo_batch_padded_records.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_compact_records.argtypes = [fp, C.c_int, C.c_int, fp, ip]
    L.cvo_gather_results_padded.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int, ip, C.c_int, ip, C.POINTER(vp)]
    L.cvo_multi_align_async_v.argtypes = [vp, ip]
    L.cvo_batch_done.argtypes = [vp, ip]
    L.cvo_batch_set_tail_scores.argtypes = [vp, C.c_int]
    L.cvo_batch_last_tail_answers.argtypes = [vp, C.c_int, ip]
    L.cvo_batch_last_pair_seconds.argtypes = [vp, C.c_int, dp]
    L.cvo_set_tail_scores.argtypes = [vp, C.c_int]
    L.cvo_batch_last_tail_seconds.argtypes = [vp, dp]
    L.cvo_batch_last_pair_spans.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_int)]
    L.cvo_batch_last_cull_masks.argtypes = [vp, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.cvo_batch_last_nonzeros.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.cvo_tracks_create.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_tracks_destroy.argtypes = [vp]
    L.cvo_tracks_set_num_want.argtypes = [vp, C.c_int]
    L.cvo_tracks_set_arith_mode.argtypes = [vp, C.c_int]
    L.cvo_tracks_reset.argtypes = [vp, C.c_int]
    L.cvo_tracks_step_async.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Camera), ip, vp]
    L.cvo_tracks_done.argtypes = [vp, ip]
    L.cvo_tracks_wait.argtypes = [vp, C.POINTER(TrackStep), C.c_int]
    L.cvo_tracks_commit.argtypes = [vp, C.c_int, ip, ip]
    L.cvo_tracks_get_cloud.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, ip]
    L.cvo_tracks_get_selected_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, ip]
    L.cvo_tracks_get_state.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, fp]
    L.cvo_batch_stage_images.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Camera), ip]
    L.cvo_batch_advance_staged.argtypes = [vp, ip]
    L.cvo_batch_staged_count.argtypes = [vp, ip, C.POINTER(C.c_longlong)]
    L.cvo_tracks_stage_async.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Camera), ip]
    L.cvo_tracks_step_staged_async.argtypes = [vp, vp]
    L.cvo_tracks_staged_count.argtypes = [vp, ip, C.POINTER(C.c_longlong)]
    dip = C.POINTER(DeviceImage)
    L.cvo_check_device_images.argtypes = [C.c_int, C.c_int, dip, C.c_int, C.c_int]
    L.cvo_selftest_ingest_images.argtypes = [C.c_int, C.c_int, dip, C.c_int, C.c_int, vp, vp, ip]
    L.cvo_batch_set_pairs_device_images.argtypes = [vp, C.c_int, C.c_int, C.c_int, dip, C.c_int, C.c_int, C.POINTER(Camera), ip, ip, ip, vp]
    L.cvo_batch_advance_device_images.argtypes = [vp, C.c_int, ip, dip, C.c_int, C.c_int, C.POINTER(Camera), ip, ip, vp]
    L.cvo_batch_stage_device_images.argtypes = [vp, C.c_int, ip, dip, C.c_int, C.c_int, C.POINTER(Camera), ip, vp]
    L.cvo_tracks_step_device_async.argtypes = [vp, C.c_int, ip, dip, C.c_int, C.c_int, C.POINTER(Camera), ip, vp, vp]
    L.cvo_tracks_stage_device_async.argtypes = [vp, C.c_int, ip, dip, C.c_int, C.c_int, C.POINTER(Camera), ip, vp]
    dcp = C.POINTER(DeviceCloud)
    L.cvo_check_device_clouds.argtypes = [C.c_int, C.c_int, dcp]
    L.cvo_selftest_ingest_clouds.argtypes = [C.c_int, C.c_int, dcp, vp, vp, vp, ip]
    L.cvo_batch_set_pairs_device_clouds.argtypes = [vp, C.c_int, C.c_int, C.c_int, dcp, ip, ip, vp]
    L.cvo_batch_advance_device_clouds.argtypes = [vp, C.c_int, ip, dcp, vp]
    L.cvo_tracks_step_device_clouds_async.argtypes = [vp, C.c_int, ip, dcp, vp, vp]
    psp = C.POINTER(PointSupportDst)
    L.cvo_point_support.argtypes = [vp, C.c_int, fp, C.c_int, fp, ip, C.c_int, fp, ip, C.c_int]
    L.cvo_batch_point_support.argtypes = [vp, C.c_int, ip, psp]
    L.cvo_batch_point_support_device.argtypes = [vp, C.c_int, ip, psp, vp]
    L.cvo_tracks_point_support.argtypes = [vp, C.c_int, C.c_int, ip, psp]
    L.cvo_tracks_point_support_device.argtypes = [vp, C.c_int, C.c_int, ip, psp, vp]
    pmp = C.POINTER(PointMatchesDst)
    L.cvo_point_matches.argtypes = [vp, C.c_int, fp, C.c_int, pmp, C.c_int, C.c_int]
    L.cvo_batch_point_matches.argtypes = [vp, C.c_int, ip, pmp]
    L.cvo_batch_point_matches_device.argtypes = [vp, C.c_int, ip, pmp, vp]
    L.cvo_tracks_point_matches.argtypes = [vp, C.c_int, C.c_int, ip, pmp]
    L.cvo_tracks_point_matches_device.argtypes = [vp, C.c_int, C.c_int, ip, pmp, vp]
    inp = C.POINTER(InnP)
    L.cvo_score_hypotheses.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, C.c_float, inp, ip]
    L.cvo_batch_score_hypotheses.argtypes = [vp, C.c_int, ip, C.c_int, fp, C.c_float, inp, ip]
    L.cvo_batch_seed_hypotheses_async.argtypes = [vp, C.c_int, ip, C.c_int, fp, C.c_float]
    L.cvo_batch_hypothesis_results.argtypes = [vp, C.c_int, inp, ip]
    pmp = C.POINTER(PoseModel)
    L.cvo_pose_models.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, C.c_float, pmp]
    L.cvo_batch_pose_models.argtypes = [vp, C.c_int, ip, C.c_int, fp, C.c_float, pmp]
    L.cvo_batch_result_models.argtypes = [vp, C.c_int, ip, pmp]
    rpp = C.POINTER(ReduceParams); rcp = C.POINTER(ReducedCloud)
    L.cvo_reducer_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.cvo_reducer_destroy.argtypes = [vp]
    L.cvo_reducer_info.argtypes = [vp, ip, ip, C.POINTER(C.c_longlong)]
    L.cvo_check_reduce_clouds.argtypes = [vp, C.c_int, dcp, rpp, rcp]
    L.cvo_reduce_device_clouds.argtypes = [vp, C.c_int, dcp, rpp, rcp, ip, vp]
    L.cvo_count_voxels.argtypes = [vp, C.c_int, dcp, C.c_int, fp, C.c_int, ip, vp]
    fmp = C.POINTER(FuseMember); fpp = C.POINTER(FuseParams); fcp = C.POINTER(FusedCloud)
    L.cvo_check_fuse_clouds.argtypes = [vp, C.c_int, ip, fmp, fpp, fcp]
    L.cvo_fuse_device_clouds.argtypes = [vp, C.c_int, ip, fmp, fpp, fcp, ip, vp]
    cap_ = C.POINTER(Camera); frame = [vp, C.c_int, dip, C.c_int, C.c_int, C.c_int, cap_, ip]   # r, count, images, width, height, step, cams, cam_index
    L.cvo_check_device_frames.argtypes = frame
    L.cvo_frames_to_device_clouds.argtypes = frame + [C.POINTER(FrameCloud), vp]
    L.cvo_reduce_device_frames.argtypes = frame + [rpp, rcp, ip, vp]
    L.cvo_count_frame_voxels.argtypes = frame + [C.c_int, fp, C.c_int, ip, vp]
    ffp = C.POINTER(FuseFrame)
    L.cvo_check_fuse_frames.argtypes = [vp, C.c_int, ip, ffp, C.c_int, C.c_int, C.c_int, cap_, fpp, fcp]
    L.cvo_fuse_device_frames.argtypes = [vp, C.c_int, ip, ffp, C.c_int, C.c_int, C.c_int, cap_, fpp, fcp, ip, vp]
    vwp = C.POINTER(View); vpp = C.POINTER(ViewParams); vcp = C.POINTER(ViewedCloud)
    L.cvo_check_view_clouds.argtypes = [vp, C.c_int, vwp, cap_, vpp, dip, vcp]
    L.cvo_view_device_clouds.argtypes = [vp, C.c_int, vwp, cap_, vpp, dip, vcp, ip, ip, vp]
    mfp = C.POINTER(MapFilter); mkp = C.POINTER(MapKeep); mcp = C.POINTER(MapCloud); vpp_ = C.POINTER(vp)
    L.cvo_maps_create.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.POINTER(vp)]
    L.cvo_maps_destroy.argtypes = [vp]
    L.cvo_maps_info.argtypes = [vp, ip, ip, fp, C.POINTER(C.c_longlong)]
    L.cvo_maps_clear.argtypes = [vp, C.c_int, ip, vp]
    L.cvo_maps_rows.argtypes = [vp, C.c_int, ip, ip, ip]
    L.cvo_check_maps_integrate_clouds.argtypes = [vp, C.c_int, ip, ip, fmp, ip, C.c_int]
    L.cvo_maps_integrate_clouds.argtypes = [vp, C.c_int, ip, ip, fmp, ip, C.c_int, vp]
    L.cvo_check_maps_integrate_frames.argtypes = [vp, C.c_int, ip, ip, ffp, C.c_int, C.c_int, C.c_int, cap_, ip, C.c_int]
    L.cvo_maps_integrate_frames.argtypes = [vp, C.c_int, ip, ip, ffp, C.c_int, C.c_int, C.c_int, cap_, ip, C.c_int, vp]
    L.cvo_check_maps_extract.argtypes = [vp, C.c_int, ip, mfp, mcp]
    L.cvo_maps_extract.argtypes = [vp, C.c_int, ip, mfp, mcp, ip, vp]
    L.cvo_check_maps_compact.argtypes = [vp, C.c_int, ip, mkp, vpp_, vpp_]
    L.cvo_maps_compact.argtypes = [vp, C.c_int, ip, mkp, vpp_, vpp_, ip, vp]
    mvp = C.POINTER(MapView)
    L.cvo_check_maps_view.argtypes = [vp, C.c_int, mvp, cap_, vpp, dip, vcp, vpp_]
    L.cvo_maps_view.argtypes = [vp, C.c_int, mvp, cap_, vpp, dip, vcp, vpp_, ip, ip, vp]
    mpp = C.POINTER(MapProbe); ppp = C.POINTER(ProbedPoints)
    L.cvo_check_maps_probe_clouds.argtypes = [vp, C.c_int, mpp, fmp, ppp]
    L.cvo_maps_probe_clouds.argtypes = [vp, C.c_int, mpp, fmp, ppp, ip, vp]
    L.cvo_check_maps_probe_frames.argtypes = [vp, C.c_int, mpp, ffp, C.c_int, C.c_int, C.c_int, cap_, ppp]
    L.cvo_maps_probe_frames.argtypes = [vp, C.c_int, mpp, ffp, C.c_int, C.c_int, C.c_int, cap_, ppp, ip, vp]
    msp = C.POINTER(MapSnapshot)
    L.cvo_check_maps_snapshot.argtypes = [vp, C.c_int, ip, msp]
    L.cvo_maps_snapshot.argtypes = [vp, C.c_int, ip, msp, ip, vp]
    L.cvo_check_maps_restore.argtypes = [vp, C.c_int, ip, msp, C.c_float]
    L.cvo_maps_restore.argtypes = [vp, C.c_int, ip, msp, C.c_float, vp]
    L.cvo_check_maps_merge.argtypes = [vp, C.c_int, C.POINTER(MapMerge), vp, C.c_int]
    L.cvo_maps_merge.argtypes = [vp, C.c_int, C.POINTER(MapMerge), vp, C.c_int, vp]
    _lib = L
    return L


def adaptive_default_params() -> AdaptiveParams:
    p = AdaptiveParams(); _check(load_library().cvo_adaptive_default_params(C.byref(p))); return p


def adaptive_align(fixed_xyz, fixed_feat, moving_xyz, moving_feat, params: AdaptiveParams | None = None, R=None, T=None, trace_cap: int = 0, device: int = 0):
    """acvo::align (adaptive_cvo.cpp:490-555) on the GPU from a fresh object: dict(transform, R, T, ell, iter, trace)."""
    L = load_library()
    p = params or adaptive_default_params()
    fx, fxp, ff, ffp = _cloud_args(fixed_xyz, fixed_feat); mx, mxp, mf, mfp = _cloud_args(moving_xyz, moving_feat)
    Rb = np.ascontiguousarray(np.eye(3) if R is None else R, np.float32).reshape(9).copy(); Tb = np.ascontiguousarray(np.zeros(3) if T is None else T, np.float32).copy()
    tf = np.zeros(12, np.float32); ell = C.c_float(0); it = C.c_int(-1); n = C.c_int(0)
    rows = (AdaptiveRow * max(1, trace_cap))()
    fp = C.POINTER(C.c_float)
    _check(L.cvo_adaptive_align(device, C.byref(p), fxp, ffp, fx.shape[0], mxp, mfp, mx.shape[0], Rb.ctypes.data_as(fp), Tb.ctypes.data_as(fp), C.byref(ell),
                                tf.ctypes.data_as(fp), C.byref(it), rows if trace_cap else None, trace_cap, C.byref(n)))
    tr = [dict(omega=np.array(r.omega[:], np.float32), v=np.array(r.v[:], np.float32), dl=r.dl, ell=r.ell, step=r.step,
               nnz_xy=r.nnz_xy, nnz_xx=r.nnz_xx, nnz_yy=r.nnz_yy) for r in rows[: n.value]]
    return dict(transform=tf.reshape(3, 4), R=Rb.reshape(3, 3), T=Tb, ell=ell.value, iter=it.value, trace=tr)


def selftest_cubic_step(coef_minstep, device: int = 0):
    """cubic_step on the device for n x {c3, c2, c1, c0, min_step} (cvo.cpp:76-92,317-333)."""
    a = np.ascontiguousarray(coef_minstep, np.float32).reshape(-1, 5); out = np.zeros(a.shape[0], np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_cubic_step(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def selftest_exp_sek3(omega_v_dt, device: int = 0):
    """Exp_SEK3 on the device for n x {omega, v, dt} (LieGroup.cpp:159-186): (n,3,3) dR and (n,3) dT."""
    a = np.ascontiguousarray(omega_v_dt, np.float32).reshape(-1, 7); out = np.zeros((a.shape[0], 12), np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_exp_sek3(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out[:, :9].reshape(-1, 3, 3), out[:, 9:]


def selftest_dist_se3(dR_dT, device: int = 0):
    """dist_se3 on the device for n x {dR row-major, dT} (cvo.cpp:94-104)."""
    a = np.ascontiguousarray(dR_dT, np.float32).reshape(-1, 12); out = np.zeros(a.shape[0], np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_dist_se3(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def selftest_cubic_step_f32eig(coef_minstep, device: int = 0):
    """cubic_step_f32eig on the device (CVO_ARITH_F32_ROOTS: the f32 companion-matrix eigenvalues) for n x {c3, c2, c1, c0, min_step}."""
    a = np.ascontiguousarray(coef_minstep, np.float32).reshape(-1, 5); out = np.zeros(a.shape[0], np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_cubic_step_f32eig(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def selftest_dist_se3_f32logm(dR_dT, device: int = 0):
    """dist_se3_f32logm on the device (CVO_ARITH_F32_LOGM: the f32 matrix logarithm's norm) for n x {dR row-major, dT}; NaN where the logarithm fails."""
    a = np.ascontiguousarray(dR_dT, np.float32).reshape(-1, 12); out = np.zeros(a.shape[0], np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_dist_se3_f32logm(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def selftest_reset_initial(transform, odometry, device: int = 0):
    """cvo::reset_initial (cvo.cpp:611-618) on the device, as the tracker streams' link kernel evaluates it, for n objects with the given
    `transform` (n, 3, 4) and odometry transforms (n, 3, 4): R (n, 3, 3), T (n, 3) and the returned init.inverse() (n, 3, 4)."""
    a = np.ascontiguousarray(np.concatenate([np.asarray(transform, np.float32).reshape(-1, 12), np.asarray(odometry, np.float32).reshape(-1, 12)], axis=1))
    out = np.zeros((a.shape[0], 24), np.float32); fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_reset_initial(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out[:, :9].reshape(-1, 3, 3), out[:, 9:12].copy(), out[:, 12:].reshape(-1, 3, 4)


def selftest_libm(x, device: int = 0):
    """The device's float routines element by element: (n, 6) = OCML sinf, cosf, logf, then the correctly rounded sine, cosine (exp_sek3) and logarithm (gates)."""
    a = np.ascontiguousarray(x, np.float32).reshape(-1); out = np.zeros((a.shape[0], 6), np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_libm(device, a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def selftest_pair_values(y_g, ell: float, params: "Params | None" = None, device: int = 0):
    """The pair arithmetic of se_kernel (cvo.cpp:166-175) on the device by the align kernel's four routes, for n x {y[3], g[5]} against a fixed
    point at the origin with zero features: (a (n, 4), d2 (n,), d2c (n,))."""
    a = np.ascontiguousarray(y_g, np.float32).reshape(-1, 8); out = np.zeros((a.shape[0], 4), np.float32); aux = np.zeros((a.shape[0], 2), np.float32)
    fp = C.POINTER(C.c_float)
    _check(load_library().cvo_selftest_pair_values(device, C.byref(params) if params is not None else None, float(ell), a.shape[0], a.ctypes.data_as(fp),
                                                   out.ctypes.data_as(fp), aux.ctypes.data_as(fp)))
    return out, aux[:, 0], aux[:, 1]


def selftest_voxel_slots(xyz, voxel: float, slots: int, device: int = 0):
    """The voxel table's two pure functions on the device (cell_of with zero features, home_slot) for n positions: (valid (n,) bool, key (n,) uint64,
    home slot (n,) uint32); key and slot are 0 for an invalid point."""
    a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); n = a.shape[0]
    valid = np.zeros(n, np.int32); key = np.zeros(n, np.uint64); slot = np.zeros(n, np.uint32)
    _check(load_library().cvo_selftest_voxel_slots(device, n, a.ctypes.data_as(C.POINTER(C.c_float)), float(voxel), int(slots),
                                                   valid.ctypes.data_as(C.POINTER(C.c_int)), key.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                   slot.ctypes.data_as(C.POINTER(C.c_uint))))
    return valid != 0, key, slot


def _check(rc: int):
    if rc != CVO_OK:
        raise CvoError(rc, load_library().cvo_last_error().decode())


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _tran(t):
    if t is None:
        return None, None
    return _f(np.asarray(t, dtype=np.float32).reshape(12))


def _inn_arrays(recs, shape):
    """an array of cvo_inn_p as (values float32, nums int32) of `shape`"""
    raw = np.frombuffer(recs, dtype=np.dtype([("value", np.float32), ("num", np.int32), ("num_e", np.int32)]))
    return raw["value"].reshape(shape).copy(), raw["num"].reshape(shape).copy()


def _model_arrays(recs, shape):
    """an array of cvo_pose_model as (values float32, nums int32, grads float64[.., 6], hess float64[.., 6, 6]) of `shape`"""
    raw = np.frombuffer(recs, dtype=np.dtype([("value", np.float32), ("num", np.int32), ("grad", np.float64, (6,)), ("hess", np.float64, (6, 6))]))
    return (raw["value"].reshape(shape).copy(), raw["num"].reshape(shape).copy(), raw["grad"].reshape(shape + (6,)).copy(),
            raw["hess"].reshape(shape + (6, 6)).copy())


def _hyp_trans(trans, count):
    """count x K x 3 x 4 transforms (a single pair may leave the first axis out) as one contiguous float32 array and K"""
    t = np.ascontiguousarray(trans, dtype=np.float32)
    if count is None:
        t = t.reshape((1,) + t.shape) if t.ndim == 3 else t
        count = t.shape[0]
    if t.ndim < 2 or t.size == 0 or t.size % (12 * count) != 0:
        raise ValueError("trans: count x K transforms of 3 x 4 expected")
    return t.reshape(count, -1, 12), t.size // (12 * count)


def default_params() -> Params:
    p = Params(); _check(load_library().cvo_default_params(C.byref(p))); return p


def device_count() -> int:
    return int(load_library().cvo_device_count())


def _cloud_args(xyz, feat):
    x, xp = _f(xyz); f, fpt = _f(feat)
    if x.ndim != 2 or x.shape[1] != 3 or f.shape != (5, x.shape[0]):
        raise ValueError("cloud must be xyz (n,3) and feat (5,n)")
    return x, xp, f, fpt


# ---- frames in device memory: anything that carries __cuda_array_interface__ (torch ROCm tensors do; torch itself is not needed here)
def is_device_image(a) -> bool:
    return hasattr(a, "__cuda_array_interface__")


def _strides_of(cai, itemsize):
    shape = tuple(int(v) for v in cai["shape"])
    st = cai.get("strides")
    if st is None:                                   # C-contiguous
        st, acc = [], itemsize
        for d in reversed(shape):
            st.append(acc); acc *= d
        st = tuple(reversed(st))
    return shape, tuple(int(v) for v in st)


def device_image(bgr, depth, swap_rb: bool = False):
    """(DeviceImage, width, height) of a frame in device memory, from the shape and strides of its two __cuda_array_interface__ carriers.
    bgr: uint8 (h, w, 3) or (h, w, 4), channel stride 1, pixel stride 3 or 4 bytes, any row stride >= the row's bytes (so a crop of a larger
    tensor, or the first three channels of a BGRA tensor, is fine as it is).  depth: uint16 or int16 (reinterpreted) (h, w), element stride 2.
    swap_rb: the colour bytes are R, G, B.  Anything else raises ValueError."""
    if not is_device_image(bgr) or not is_device_image(depth):
        raise ValueError("a device image is a pair of objects with __cuda_array_interface__")
    cb, cd = bgr.__cuda_array_interface__, depth.__cuda_array_interface__
    if cb["typestr"] != "|u1":
        raise ValueError(f"bgr: uint8 expected, got typestr {cb['typestr']!r}")
    if cd["typestr"] not in ("<u2", "<i2"):
        raise ValueError(f"depth: little-endian uint16 or int16 expected, got typestr {cd['typestr']!r}")
    sb, tb = _strides_of(cb, 1)
    sd, td = _strides_of(cd, 2)
    if len(sb) != 3 or sb[2] not in (3, 4):
        raise ValueError(f"bgr: shape (h, w, 3) or (h, w, 4) expected, got {sb}")
    h, w = sb[0], sb[1]
    if tb[2] != 1:
        raise ValueError(f"bgr: channel stride 1 expected, got {tb[2]}")
    if tb[1] not in (3, 4) or tb[1] < sb[2]:
        raise ValueError(f"bgr: pixel stride 3 or 4 bytes expected, got {tb[1]} for {sb[2]} channels")
    if tb[0] < w * tb[1]:
        raise ValueError(f"bgr: row stride {tb[0]} is below the row's {w * tb[1]} bytes")
    if len(sd) != 2 or sd != (h, w):
        raise ValueError(f"depth: shape {(h, w)} expected, got {sd}")
    if td[1] != 2:
        raise ValueError(f"depth: element stride 2 bytes expected, got {td[1]}")
    if td[0] < 2 * w:
        raise ValueError(f"depth: row stride {td[0]} is below the row's {2 * w} bytes")
    pb, pd = cb["data"][0], cd["data"][0]
    if not pb or not pd:
        raise ValueError("null device pointer")
    return DeviceImage(pb, pd, tb[0], td[0], tb[1], 1 if swap_rb else 0), w, h


def _images_on_device(images) -> bool:
    """True: every image of the list is a device image; False: none is.  A mixed list raises ValueError."""
    kinds = {bool(is_device_image(b)) and bool(is_device_image(d)) for b, d in images}
    if len(kinds) > 1 or any(is_device_image(b) != is_device_image(d) for b, d in images):
        raise ValueError("host and device images mixed in one call")
    return bool(kinds) and kinds.pop()


def _device_images(images, swap_rb):
    """[(DeviceImage, w, h)] of a list of (bgr, depth) device images; swap_rb: one flag for all, or one per image"""
    sw = list(swap_rb) if hasattr(swap_rb, "__len__") else [swap_rb] * len(images)
    if len(sw) != len(images):
        raise ValueError("swap_rb: one flag, or one per image")
    return [device_image(b, d, bool(f)) for (b, d), f in zip(images, sw)]


def _stream_arg(image_stream):
    h = getattr(image_stream, "cuda_stream", image_stream)   # a torch.cuda.Stream, or a raw hipStream_t value
    return C.c_void_p(int(h)) if h else None


def _settle_writer(images, image_stream):
    """image_stream None: the entry point takes the images as already written.  torch tensors are written on torch's current stream, so that
    stream is synchronised first (torch is only looked at when the caller has loaded it)."""
    if image_stream is not None or "torch" not in sys.modules:
        return
    torch = sys.modules["torch"]
    t = images[0][0]
    if isinstance(t, torch.Tensor) and t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()


def _device_list_args(ids, images, cameras, cam_index, what, swap_rb):
    """_image_list_args for device images: (n, ids, descriptors, w, h, cameras, cam_index or None) plus what must stay alive"""
    ims = _device_images(images, swap_rb)
    sl = np.ascontiguousarray(ids, np.int32).reshape(-1)
    if not ims or sl.shape[0] != len(ims):
        raise ValueError(f"one {what} per image, at least one image")
    w, h = ims[0][1], ims[0][2]
    if any((q[1], q[2]) != (w, h) for q in ims):
        raise ValueError("all images of one call must have the same size")
    if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
        cameras = [cameras]
    cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
    ci = None if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
    if ci is not None and (ci.shape[0] != len(ims) or ci.min() < 0 or ci.max() >= len(cameras)):
        raise ValueError("cam_index: one index into cameras per image")
    n = len(ims); ip = C.POINTER(C.c_int)
    descs = (DeviceImage * n)(*[q[0] for q in ims])
    return (n, sl.ctypes.data_as(ip), descs, w, h, cams, None if ci is None else ci.ctypes.data_as(ip)), (sl, ci, images)


def check_device_images(images, swap_rb: bool = False, device: int = 0):
    """cvo_check_device_images: the validation every device entry point runs first, alone (nothing is launched).  images: a list of
    (bgr, depth) device images of one size.  Raises CvoError (code 4, the message names image and field) for what the device cannot read."""
    ims = _device_images(images, swap_rb)
    descs = (DeviceImage * len(ims))(*[q[0] for q in ims])
    _check(load_library().cvo_check_device_images(device, len(ims), descs, ims[0][1], ims[0][2]))


def selftest_ingest_images(descs, width: int, height: int, device: int = 0):
    """cvo_selftest_ingest_images: the ingest kernel alone on a list of DeviceImage; returns (bgr stack (count, h, w, 3) uint8,
    depth stack (count, h, w) uint16, guards intact)"""
    n = len(descs)
    arr = (DeviceImage * n)(*descs)
    bgr = np.zeros((n, height, width, 3), np.uint8); dep = np.zeros((n, height, width), np.uint16); ok = C.c_int(0)
    _check(load_library().cvo_selftest_ingest_images(device, n, arr, int(width), int(height), bgr.ctypes.data, dep.ctypes.data, C.byref(ok)))
    return bgr, dep, bool(ok.value)


# ---- clouds in device memory (cvo_hip.h: cvo_device_cloud): the same carriers
def device_cloud(xyz, feat, feat_layout: str | None = None, max_n: int = 65535) -> DeviceCloud:
    """DeviceCloud of a cloud in device memory, from the shape and strides of its two __cuda_array_interface__ carriers.
    max_n: the most points the receiver takes: 65535 for a hand-over, up to REDUCE_MAX_POINTS in front of a CvoReducer.
    xyz: float32 (n, 3), inner stride 4 bytes, any row stride that is a multiple of 4 and at least 12 (a slice of a wider tensor, float4 points).
    feat: float32 (5, n) (channels first) or (n, 5) (points first), told apart by the shape; a 5 x 5 tensor needs feat_layout = "channels_first"
    or "points_first".  Strides must be positive multiples of 4.  Anything else -- a host array among it -- raises ValueError."""
    if not hasattr(xyz, "__cuda_array_interface__") or not hasattr(feat, "__cuda_array_interface__"):
        raise ValueError("a device cloud is a pair of objects with __cuda_array_interface__ (a host array is handed over with set_pairs / set_pcd)")
    if feat_layout not in (None, "channels_first", "points_first"):
        raise ValueError(f"feat_layout: 'channels_first' or 'points_first' expected, got {feat_layout!r}")
    cx, cf = xyz.__cuda_array_interface__, feat.__cuda_array_interface__
    for name, c in (("xyz", cx), ("feat", cf)):
        if c["typestr"] != "<f4":
            raise ValueError(f"{name}: little-endian float32 expected, got typestr {c['typestr']!r}")
    sx, tx = _strides_of(cx, 4)
    sf, tf = _strides_of(cf, 4)
    if len(sx) != 2 or sx[1] != 3:
        raise ValueError(f"xyz: shape (n, 3) expected, got {sx}")
    n = sx[0]
    if len(sf) != 2 or 5 not in sf:
        raise ValueError(f"feat: shape (5, n) or (n, 5) expected, got {sf}")
    if sf == (5, 5) and feat_layout is None:
        raise ValueError("feat: a 5 x 5 tensor reads either way, say feat_layout = 'channels_first' or 'points_first'")
    channels_first = (feat_layout == "channels_first") if feat_layout else sf[0] == 5
    if sf !=((5, n) if channels_first else (n, 5)):
        raise ValueError(f"feat: shape {(5, n) if channels_first else (n, 5)} expected for {n} points, got {sf}")
    if n > max_n:
        raise ValueError(f"{n} points: more than {max_n} per cloud is not supported")
    if n == 0:
        return DeviceCloud(None, None, 0, 0, 0, 0, 0)
    point_stride, channel_stride = (tf[1], tf[0]) if channels_first else (tf[0], tf[1])
    if tx[1] != 4:
        raise ValueError(f"xyz: inner stride 4 bytes expected, got {tx[1]}")
    for name, v in (("xyz row", tx[0]), ("feat point", point_stride), ("feat channel", channel_stride)):
        if v <= 0:
            raise ValueError(f"{name} stride {v}: a positive stride expected")
        if v % 4:
            raise ValueError(f"{name} stride {v} is not a multiple of 4")
    if tx[0] < 12:
        raise ValueError(f"xyz row stride {tx[0]} is below a point's 12 bytes")
    px, pf = cx["data"][0], cf["data"][0]
    if not px or not pf:
        raise ValueError("null device pointer")
    if px % 4 or pf % 4:
        raise ValueError("a base pointer is not 4-byte aligned")
    return DeviceCloud(px, pf, tx[0], point_stride, channel_stride, n, 0)


def _device_clouds(clouds, max_n: int = 65535):
    """(ctypes array of DeviceCloud, n) of a list whose entries are DeviceCloud, (xyz, feat) or (xyz, feat, feat_layout)"""
    ds = [c if isinstance(c, DeviceCloud) else device_cloud(*c, max_n=max_n) for c in clouds]
    if not ds:
        raise ValueError("no clouds")
    return (DeviceCloud * len(ds))(*ds), len(ds)


def _settle_cloud_writer(clouds, cloud_stream):
    first = next((c for c in clouds if not isinstance(c, DeviceCloud)), None)
    if first is not None:
        _settle_writer([(first[0], None)], cloud_stream)


def check_device_clouds(clouds, device: int = 0):
    """cvo_check_device_clouds: the validation every device-cloud entry point runs first, alone (nothing is launched).  clouds: a list of
    DeviceCloud, (xyz, feat) or (xyz, feat, feat_layout).  Raises CvoError (code 4, the message names cloud and field)."""
    arr, n = _device_clouds(clouds)
    _check(load_library().cvo_check_device_clouds(device, n, arr))


def selftest_ingest_clouds(clouds, device: int = 0):
    """cvo_selftest_ingest_clouds: the ingest kernel alone.  Returns ([(xyz (n, 3), feat (5, n)) per cloud], cost (count, 2) float64 {sum,
    samples}, guards intact)."""
    arr, n = _device_clouds(clouds)
    ns = [int(arr[k].n) for k in range(n)]
    tot = sum(ns)
    xyz = np.zeros(max(1, 3 * tot), np.float32); feat = np.zeros(max(1, 5 * tot), np.float32); cost = np.zeros((n, 2), np.float64); ok = C.c_int(0)
    _check(load_library().cvo_selftest_ingest_clouds(device, n, arr, xyz.ctypes.data, feat.ctypes.data, cost.ctypes.data, C.byref(ok)))
    out, at = [], 0
    for m in ns:
        out.append((xyz[3 * at:3 * (at + m)].reshape(m, 3).copy(), feat[5 * at:5 * (at + m)].reshape(5, m).copy()))
        at += m
    return out, cost, bool(ok.value)


# ---- reducing clouds (cvo_hip.h, "Reducing clouds"): a voxel-grid filter in front of the device-cloud hand-over
class CvoReducer:
    """cvo_reducer: reduces clouds in device memory to one row per occupied voxel, many clouds per call, the result's bits a function of the
    input alone.  max_clouds, max_points: the most clouds per call and points per cloud (up to REDUCE_MAX_POINTS); the device scratch, 384
    bytes per point of max_clouds x max_points, is allocated here and never grows.  Outputs are torch tensors on the reducer's device.
    `fuse` (cvo_hip.h, "Fusing clouds") runs groups of posed clouds through the same machinery, on the same scratch: max_clouds groups per
    call, max_points points per group.  `view` (cvo_hip.h, "Viewing clouds") renders posed clouds at a camera on the same scratch: max_clouds
    views per call, max_points points per cloud and z-cells per image."""

    def __init__(self, max_clouds: int, max_points: int, device: int = 0):
        self.L = load_library()
        self.max_clouds, self.max_points, self.device = int(max_clouds), int(max_points), int(device)
        self.h = C.c_void_p()
        _check(self.L.cvo_reducer_create(self.device, self.max_clouds, self.max_points, C.byref(self.h)))

    def close(self):
        """cvo_reducer_destroy.  Raises CvoError, and keeps the reducer, while CvoMaps objects created on it are open: close those first."""
        if getattr(self, "h", None) and self.h.value:
            _check(self.L.cvo_reducer_destroy(self.h)); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scratch_bytes(self) -> int:
        b = C.c_longlong(0)
        _check(self.L.cvo_reducer_info(self.h, None, None, C.byref(b)))
        return b.value

    def _inputs(self, clouds, cloud_stream):
        arr, n = _device_clouds(clouds, max_n=REDUCE_MAX_POINTS)
        _settle_cloud_writer(clouds, cloud_stream)
        return arr, n

    def reduce(self, clouds, voxel: float, mode="mean", min_points: int = 1, cap: int = 65535, want=("count",), cloud_stream=None):
        """cvo_reduce_device_clouds.  clouds: what set_pairs_clouds takes (DeviceCloud, (xyz, feat) or (xyz, feat, feat_layout)), up to
        max_points points each.  mode: "mean" or "central".  cap: the most rows a cloud may come to (at most 65535, what a hand-over takes).
        want: which of "count", "source", "map" to return beside xyz and feat.  cloud_stream: the stream that wrote the clouds; the outputs are
        ordered on it (None: torch's current stream is synchronised first and everything is done on return).
        Returns one dict per cloud: xyz (n_out, 3) and feat (n_out, 5) float32, count / source (n_out,) int32, map (n,) int32, n_out.  The
        tensors are views of the arrays the kernel wrote and pass into device_cloud / set_pairs_clouds / advance_clouds / step_clouds as they
        are.  Raises CvoError when a cloud has more than cap rows (then nothing is returned; count_voxels / voxel_for_budget choose a size)."""
        self._reduce_args(mode, want)
        arr, n = self._inputs(clouds, cloud_stream)
        ns = [int(arr[k].n) for k in range(n)]
        call = lambda prm, recs, n_out: self.L.cvo_reduce_device_clouds(self.h, n, arr, C.byref(prm), recs, n_out, _stream_arg(cloud_stream))
        return self._run_reduce(call, ns, voxel, mode, min_points, cap, want, cloud_stream, "cloud", "voxel_for_budget", False)

    @staticmethod
    def _reduce_args(mode, want):
        bad = [w for w in want if w not in ("count", "source", "map")]
        if bad:
            raise ValueError(f"want: 'count', 'source' or 'map' expected, got {bad[0]!r}")
        if mode not in REDUCE_MODES and mode not in REDUCE_MODES.values():
            raise ValueError(f"mode: 'mean' or 'central' expected, got {mode!r}")

    def _run_reduce(self, call, ns, voxel, mode, min_points, cap, want, cloud_stream, what, helper, count_only):
        """the output arrays of a reduction of len(ns) clouds of ns points, the call, and the per-cloud dicts.  count_only: cap == 0 counts"""
        import torch
        n = len(ns)
        caps = [min(int(cap), m) if 0 <= int(cap) <= 65535 else int(cap) for m in ns]       # (a cap out of range is the library's to refuse)
        rows = [max(0, c) for c in caps]
        dev = torch.device("cuda", self.device)
        stream = None
        if cloud_stream is not None:
            stream = cloud_stream if isinstance(cloud_stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(cloud_stream), device=dev)
        with torch.cuda.stream(stream):                               # (the arrays belong to the stream their readers will use)
            xyz = torch.empty((sum(rows), 3), dtype=torch.float32, device=dev); feat = torch.empty((sum(rows), 5), dtype=torch.float32, device=dev)
            cnt = torch.empty(sum(rows), dtype=torch.int32, device=dev) if "count" in want else None
            src = torch.empty(sum(rows), dtype=torch.int32, device=dev) if "source" in want else None
            mp = torch.empty(sum(ns), dtype=torch.int32, device=dev) if "map" in want else None
        recs = (ReducedCloud * n)(); at = pt = 0; views = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = dict(xyz=xyz[at:at + rows[k]], feat=feat[at:at + rows[k]])
            if cnt is not None: v["count"] = cnt[at:at + rows[k]]
            if src is not None: v["source"] = src[at:at + rows[k]]
            if mp is not None: v["map"] = mp[pt:pt + ns[k]]
            recs[k] = ReducedCloud(ptr(v["xyz"]), ptr(v["feat"]), ptr(v.get("count")), ptr(v.get("source")), ptr(v.get("map")), caps[k], 0)
            views.append(v); at += rows[k]; pt += ns[k]
        prm = ReduceParams(float(voxel), int(REDUCE_MODES.get(mode, mode)), int(min_points), 0)
        n_out = np.zeros(n, np.int32)
        _check(call(prm, recs, n_out.ctypes.data_as(C.POINTER(C.c_int))))
        over = [k for k in range(n) if n_out[k] > caps[k]] if not (count_only and int(cap) == 0) else []
        if over:
            k = over[0]
            raise CvoError(CVO_ERR_INVALID, f"{what} {k}: {int(n_out[k])} rows at voxel {float(voxel):g} are more than cap {int(cap)}: choose a larger voxel ({helper})")
        out = []
        for k, v in enumerate(views):
            m = int(n_out[k])
            out.append({key: (t if key == "map" else t[:m]) for key, t in v.items()} | dict(n_out=m))
        return out

    def count_voxels(self, clouds, voxels, min_points: int = 1, cloud_stream=None):
        """cvo_count_voxels: the occupied-cell counts (count, k) int32 of every cloud at every one of the k <= 16 voxel sizes, by one call;
        counts[i, j] is what reduce would return as n_out for cloud i at voxels[j]."""
        vs = np.ascontiguousarray(voxels, np.float32).reshape(-1)
        arr, n = self._inputs(clouds, cloud_stream)
        out = np.zeros((n, vs.shape[0]), np.int32)
        _check(self.L.cvo_count_voxels(self.h, n, arr, int(vs.shape[0]), vs.ctypes.data_as(C.POINTER(C.c_float)), int(min_points),
                                       out.ctypes.data_as(C.POINTER(C.c_int)), _stream_arg(cloud_stream)))
        return out

    def _fuse_inputs(self, groups, poses, min_views, mode, want):
        """what fuse refuses before it touches the library, and its (FuseMember array, group_first, per-group member sizes)"""
        groups, poses = self._fuse_args(groups, poses, min_views, mode, want)
        members, first, sizes = [], [0], []
        for g, (clouds, ps) in enumerate(zip(groups, poses)):
            ns = []
            for c, M in zip(clouds, ps):
                d = c if isinstance(c, DeviceCloud) else device_cloud(*c, max_n=REDUCE_MAX_POINTS)
                members.append(FuseMember(d, (C.c_float * 12)(*M[:3].reshape(-1).tolist())))
                ns.append(int(d.n))
            first.append(len(members)); sizes.append(ns)
        return (FuseMember * len(members))(*members), np.asarray(first, np.int32), sizes, groups

    @staticmethod
    def _fuse_args(groups, poses, min_views, mode, want):
        """the argument checks of a fusion: (groups as lists, poses as float32 arrays)"""
        bad = [w for w in want if w not in FUSE_WANT]
        if bad:
            raise ValueError(f"want: one of {FUSE_WANT} expected, got {bad[0]!r}")
        if mode not in REDUCE_MODES and mode not in REDUCE_MODES.values():
            raise ValueError(f"mode: 'mean' or 'central' expected, got {mode!r}")
        if not 1 <= int(min_views) <= FUSE_MAX_MEMBERS:
            raise ValueError(f"min_views {min_views}: 1 .. {FUSE_MAX_MEMBERS} expected")
        groups = [list(g) for g in groups]; poses = [list(q) for q in poses]
        if not groups:
            raise ValueError("no groups")
        if len(poses) != len(groups):
            raise ValueError(f"{len(groups)} groups but {len(poses)} lists of poses")
        out = []
        for g, (clouds, ps) in enumerate(zip(groups, poses)):
            if not 1 <= len(clouds) <= FUSE_MAX_MEMBERS:
                raise ValueError(f"group {g}: {len(clouds)} members, 1 .. {FUSE_MAX_MEMBERS} expected")
            if len(ps) != len(clouds):
                raise ValueError(f"group {g}: {len(clouds)} members but {len(ps)} poses")
            Ms = []
            for m, pose in enumerate(ps):
                M = np.asarray(pose, np.float32)
                if M.shape not in ((3, 4), (4, 4)):
                    raise ValueError(f"group {g} member {m}: a 3 x 4 or 4 x 4 pose expected, got shape {M.shape}")
                if not np.isfinite(M[:3]).all():
                    raise ValueError(f"group {g} member {m}: the pose is not finite")
                Ms.append(M)
            out.append(Ms)
        return groups, out

    def fuse(self, groups, poses, voxel: float, mode="mean", min_points: int = 1, min_views: int = 1, cap: int = 65535, want=("count",), cloud_stream=None):
        """cvo_fuse_device_clouds: every group of posed clouds fused into one voxel-reduced cloud -- a local map -- by one call.  groups: a list
        of lists of what `reduce` takes for one cloud (1 .. 64 members each); poses: a matching list of lists of 3 x 4 or 4 x 4 array-likes (host;
        the last row of a 4 x 4 is ignored).  min_views: a cell is kept when at least that many members have a point in it.  want: which of
        "count", "source" (global index: split_source), "map" (one row number per global index: voxels.lift), "views", "view_mask" to return beside
        xyz and feat.  cap, mode, min_points, cloud_stream: reduce's.  Returns one dict per group, as reduce does, plus `offsets`: the members'
        base global indices (numpy int64).  Raises CvoError when a group comes to more than cap rows; cap = 0 counts only: nothing is written,
        n_out is the full row count and the arrays are empty."""
        arr, first, sizes, groups = self._fuse_inputs(groups, poses, min_views, mode, want)
        _settle_cloud_writer([c for g in groups for c in g], cloud_stream)
        call = lambda prm, recs, n_out: self.L.cvo_fuse_device_clouds(self.h, len(groups), first.ctypes.data_as(C.POINTER(C.c_int)), arr, C.byref(prm), recs,
                                                                      n_out, _stream_arg(cloud_stream))
        return self._run_fuse(call, sizes, voxel, mode, min_points, min_views, cap, want, cloud_stream, "fuse_voxel_for_budget")

    def _run_fuse(self, call, sizes, voxel, mode, min_points, min_views, cap, want, cloud_stream, helper):
        """the output arrays of a fusion of len(sizes) groups whose members have sizes[g] points, the call, and the per-group dicts"""
        import torch
        n = len(sizes)
        ns = [sum(q) for q in sizes]
        caps = [min(int(cap), m) if 0 <= int(cap) <= 65535 else int(cap) for m in ns]       # (a cap out of range is the library's to refuse)
        rows = [max(0, c) for c in caps]
        dev = torch.device("cuda", self.device)
        stream = None
        if cloud_stream is not None:
            stream = cloud_stream if isinstance(cloud_stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(cloud_stream), device=dev)
        per_row = dict(xyz=((3,), torch.float32), feat=((5,), torch.float32), count=((), torch.int32), source=((), torch.int32), views=((), torch.int32),
                       view_mask=((), torch.int64))                   # (the mask's 64 bits in torch's signed carrier: bit 63 is the sign)
        with torch.cuda.stream(stream):                               # (the arrays belong to the stream their readers will use)
            whole = {k: torch.empty((sum(rows),) + sh, dtype=dt, device=dev) for k, (sh, dt) in per_row.items() if k in ("xyz", "feat") or k in want}
            mp = torch.empty(sum(ns), dtype=torch.int32, device=dev) if "map" in want else None
        recs = (FusedCloud * n)(); at = pt = 0; views = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = {key: t[at:at + rows[k]] for key, t in whole.items()}
            if mp is not None: v["map"] = mp[pt:pt + ns[k]]
            recs[k] = FusedCloud(*[ptr(v.get(key)) for key in ("xyz", "feat", "count", "source", "map", "views", "view_mask")], caps[k], 0)
            views.append(v); at += rows[k]; pt += ns[k]
        prm = FuseParams(float(voxel), int(REDUCE_MODES.get(mode, mode)), int(min_points), int(min_views))
        n_out = np.zeros(n, np.int32)
        _check(call(prm, recs, n_out.ctypes.data_as(C.POINTER(C.c_int))))
        over = [k for k in range(n) if n_out[k] > caps[k]] if int(cap) != 0 else []      # (cap 0 counts only: n_out is the answer)
        if over:
            k = over[0]
            raise CvoError(CVO_ERR_INVALID, f"group {k}: {int(n_out[k])} rows at voxel {float(voxel):g} are more than cap {int(cap)}: choose a larger voxel ({helper})")
        out = []
        for k, v in enumerate(views):
            m = int(n_out[k])
            offsets = np.concatenate([[0], np.cumsum(sizes[k])[:-1]]).astype(np.int64)
            out.append({key: (t if key == "map" else t[:m]) for key, t in v.items()} | dict(n_out=m, offsets=offsets))
        return out

    # ---- frames read in place (cvo_hip.h, "Reducing frames"): the same calls with RGB-D frames where the clouds were
    @staticmethod
    def _frame_list(frames, cameras, cam_index, step, swap_rb):
        """what the frame calls refuse before they touch the library, and (descriptors [DeviceImage], w, h, step, Camera array, cam index per frame)"""
        frames = list(frames)
        if not frames:
            raise ValueError("no frames")
        if int(step) != step or not 1 <= int(step) <= FRAME_MAX_STEP:
            raise ValueError(f"step {step}: an integer in 1 .. {FRAME_MAX_STEP} expected")
        ims = _device_images(frames, swap_rb)
        w, h = ims[0][1], ims[0][2]
        if any((q[1], q[2]) != (w, h) for q in ims):
            raise ValueError("all frames of one call must have the same size")
        if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
            cameras = [cameras]
        cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
        ci = np.zeros(len(ims), np.int32) if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
        if ci.shape[0] != len(ims) or ci.min() < 0 or ci.max() >= len(cameras):
            raise ValueError("cam_index: one index into cameras per frame")
        return [q[0] for q in ims], w, h, int(step), cams, ci

    def _frame_inputs(self, frames, cameras, cam_index, step, swap_rb, image_stream):
        """the leading arguments of a frame call (r, count, images, width, height, step, cams, cam_index), the points per frame, what must stay alive"""
        descs, w, h, step, cams, ci = self._frame_list(frames, cameras, cam_index, step, swap_rb)
        _settle_writer(list(frames), image_stream)
        arr = (DeviceImage * len(descs))(*descs)
        n = -(-w // step) * -(-h // step)
        return (self.h, len(descs), arr, w, h, step, cams, ci.ctypes.data_as(C.POINTER(C.c_int))), n, (arr, cams, ci, frames)

    def check_frames(self, frames, cameras, cam_index=None, step: int = 1, swap_rb=False):
        """cvo_check_device_frames: the validation every frame call runs first, alone (nothing is launched)"""
        descs, w, h, step, cams, ci = self._frame_list(frames, cameras, cam_index, step, swap_rb)
        arr = (DeviceImage * len(descs))(*descs)
        _check(self.L.cvo_check_device_frames(self.h, len(descs), arr, w, h, step, cams, ci.ctypes.data_as(C.POINTER(C.c_int))))

    def dense_frames(self, frames, cameras, cam_index=None, step: int = 1, swap_rb=False, image_stream=None):
        """cvo_frames_to_device_clouds: the dense cloud of every frame -- one point per pixel of the sub-grid of `step`, n = ceil(w / step) *
        ceil(h / step), row-major; a pixel without depth is a row of NaN positions.  frames: a list of (bgr, depth) device images of one size,
        what device_image takes (torch tensors, crops, BGRA); cameras: one (scaling_factor, fx, fy, cx, cy) or a list, with cam_index one index
        per frame; swap_rb: one flag or one per frame.  Returns one (xyz (n, 3), feat (n, 5)) pair of float32 tensors per frame, which pass
        into reduce / fuse as they are.  The reduce, count and fuse calls below compute exactly what those do on these clouds, without them."""
        import torch
        args, n, keep = self._frame_inputs(frames, cameras, cam_index, step, swap_rb, image_stream)
        count = args[1]
        dev = torch.device("cuda", self.device)
        stream = None
        if image_stream is not None:
            stream = image_stream if isinstance(image_stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(image_stream), device=dev)
        with torch.cuda.stream(stream):
            xyz = torch.empty((count, n, 3), dtype=torch.float32, device=dev); feat = torch.empty((count, n, 5), dtype=torch.float32, device=dev)
        dst = (FrameCloud * count)(*[FrameCloud(xyz[k].data_ptr(), feat[k].data_ptr()) for k in range(count)])
        _check(self.L.cvo_frames_to_device_clouds(*args, dst, _stream_arg(image_stream)))
        return [(xyz[k], feat[k]) for k in range(count)]

    def reduce_frames(self, frames, cameras, voxel: float, cam_index=None, step: int = 1, mode="mean", min_points: int = 1, cap: int = 65535,
                      want=("count",), swap_rb=False, image_stream=None):
        """cvo_reduce_device_frames: `reduce` of the frames' dense clouds (dense_frames), which never exist in memory: each pixel's point is
        computed where it is needed.  frames, cameras, cam_index, step, swap_rb: dense_frames'; the rest and the result: reduce's, with map one
        row number per sub-grid pixel and source a sub-grid pixel's index i (pixel ((i % ws) * step, (i // ws) * step)).  cap = 0 counts
        only."""
        self._reduce_args(mode, want)
        args, n, keep = self._frame_inputs(frames, cameras, cam_index, step, swap_rb, image_stream)
        call = lambda prm, recs, n_out: self.L.cvo_reduce_device_frames(*args, C.byref(prm), recs, n_out, _stream_arg(image_stream))
        return self._run_reduce(call, [n] * args[1], voxel, mode, min_points, cap, want, image_stream, "frame", "frame_voxel_for_budget", True)

    def count_frame_voxels(self, frames, cameras, voxels, cam_index=None, step: int = 1, min_points: int = 1, swap_rb=False, image_stream=None):
        """cvo_count_frame_voxels: count_voxels of the frames' dense clouds: (count, k) int32, counts[i, j] what reduce_frames would return as
        n_out for frame i at voxels[j].  Reads 2 bytes per pixel and size."""
        vs = np.ascontiguousarray(voxels, np.float32).reshape(-1)
        args, n, keep = self._frame_inputs(frames, cameras, cam_index, step, swap_rb, image_stream)
        out = np.zeros((args[1], vs.shape[0]), np.int32)
        _check(self.L.cvo_count_frame_voxels(*args, int(vs.shape[0]), vs.ctypes.data_as(C.POINTER(C.c_float)), int(min_points),
                                             out.ctypes.data_as(C.POINTER(C.c_int)), _stream_arg(image_stream)))
        return out

    def fuse_frames(self, groups, poses, cameras, voxel: float, cam_index=None, step: int = 1, mode="mean", min_points: int = 1, min_views: int = 1,
                    cap: int = 65535, want=("count",), swap_rb: bool = False, image_stream=None):
        """cvo_fuse_device_frames: `fuse` of the frames' dense clouds, which never exist in memory.  groups: a list of lists of (bgr, depth)
        device images, all of one size (a keyframe window per group); poses: fuse's; cameras: one camera or a list, with cam_index a list of
        lists of indices shaped like groups.  The rest and the result: fuse's (every member has ceil(w / step) * ceil(h / step) points)."""
        groups, Ms = self._fuse_args(groups, poses, min_views, mode, want)
        flat = [f for g in groups for f in g]
        ci = None if cam_index is None else [int(c) for q in cam_index for c in q]
        descs, w, h, step, cams, ci = self._frame_list(flat, cameras, ci, step, swap_rb)
        _settle_writer(flat, image_stream)
        flat_M = [M for q in Ms for M in q]
        arr = (FuseFrame * len(descs))(*[FuseFrame(d, (C.c_float * 12)(*M[:3].reshape(-1).tolist()), int(c), 0) for d, M, c in zip(descs, flat_M, ci)])
        first = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
        n = -(-w // step) * -(-h // step)
        call = lambda prm, recs, n_out: self.L.cvo_fuse_device_frames(self.h, len(groups), first.ctypes.data_as(C.POINTER(C.c_int)), arr, w, h, step, cams,
                                                                      C.byref(prm), recs, n_out, _stream_arg(image_stream))
        return self._run_fuse(call, [[n] * len(g) for g in groups], voxel, mode, min_points, min_views, cap, want, image_stream, "a count-only fuse_frames call, cap = 0")

    # ---- viewing clouds (cvo_hip.h, "Viewing clouds"): posed clouds seen from a camera
    @staticmethod
    def _observed_depth(o, w, h, k):
        """the DeviceImage of view k's observed depth: a uint16 / int16 (h, w) device array, or a (bgr, depth) pair whose depth is taken"""
        d = o[1] if isinstance(o, (tuple, list)) else o
        if not hasattr(d, "__cuda_array_interface__"):
            raise ValueError(f"observed {k}: a depth image is an object with __cuda_array_interface__")
        cd = d.__cuda_array_interface__
        if cd["typestr"] not in ("<u2", "<i2"):
            raise ValueError(f"observed {k}: little-endian uint16 or int16 expected, got typestr {cd['typestr']!r}")
        sd, td = _strides_of(cd, 2)
        if sd != (h, w):
            raise ValueError(f"observed {k}: shape {(h, w)} expected, got {sd}")
        if td[1] != 2 or td[0] < 2 * w:
            raise ValueError(f"observed {k}: element stride 2 and a row stride of at least {2 * w} bytes expected, got {td}")
        if not cd["data"][0]:
            raise ValueError(f"observed {k}: null device pointer")
        return DeviceImage(None, cd["data"][0], 0, td[0], 3, 0)

    @staticmethod
    def _view_call(items, what, record, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, want, cam_index):
        """what a viewing call refuses before it touches the library, over its `items` (`what`: "clouds", or "maps" for CvoMaps.view);
        record(k, item, pose12, cam) makes view k's record.  (records, Camera array, ViewParams, DeviceImage array or None)"""
        bad = [w for w in want if w not in VIEW_WANT]
        if bad:
            raise ValueError(f"want: one of {VIEW_WANT} expected, got {bad[0]!r}")
        if "relation" in want and observed is None:
            raise ValueError("want: 'relation' needs observed")
        if mode not in VIEW_MODES and mode not in VIEW_MODES.values():
            raise ValueError(f"mode: 'front' or 'surface' expected, got {mode!r}")
        if int(cell) != cell or not 1 <= int(cell) <= VIEW_MAX_CELL:
            raise ValueError(f"cell {cell}: an integer in 1 .. {VIEW_MAX_CELL} expected")
        w, h = (int(v) for v in size)
        if not (1 <= w <= VIEW_MAX_SIZE and 1 <= h <= VIEW_MAX_SIZE):
            raise ValueError(f"size {(w, h)}: (width, height), each in 1 .. {VIEW_MAX_SIZE}, expected")
        near, far = (float(np.float32(v)) for v in z_range)
        if not (np.isfinite(near) and near > 0.0):
            raise ValueError(f"z_range: near {near} is not a finite depth above 0")
        if not (np.isfinite(far) and far > near and far <= 32768.0):
            raise ValueError(f"z_range: far {far} is not a finite depth above near {near} and at most 32768")
        if not (np.isfinite(slack) and slack >= 0.0):
            raise ValueError(f"slack {slack}: a finite number, at least 0, expected")
        if not (np.isfinite(depth_tol) and depth_tol >= 0.0):
            raise ValueError(f"depth_tol {depth_tol}: a finite number, at least 0, expected")
        items = list(items); poses = list(poses)
        if not items:
            raise ValueError(f"no {what}")
        if len(poses) != len(items):
            raise ValueError(f"{len(items)} {what} but {len(poses)} poses")
        if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
            cameras = [cameras]
        cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
        ci = np.zeros(len(items), np.int32) if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
        if ci.shape[0] != len(items) or ci.min() < 0 or ci.max() >= len(cameras):
            raise ValueError("cam_index: one index into cameras per view")
        views = []
        for k, (c, pose) in enumerate(zip(items, poses)):
            M = np.asarray(pose, np.float32)
            if M.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"view {k}: a 3 x 4 or 4 x 4 pose expected, got shape {M.shape}")
            if not np.isfinite(M[:3]).all():
                raise ValueError(f"view {k}: the pose is not finite")
            views.append(record(k, c, (C.c_float * 12)(*M[:3].reshape(-1).tolist()), int(ci[k])))
        obs = None
        if observed is not None:
            observed = list(observed)
            if len(observed) != len(items):
                raise ValueError(f"{len(items)} {what} but {len(observed)} observed depth images")
            obs = (DeviceImage * len(observed))(*[CvoReducer._observed_depth(o, w, h, k) for k, o in enumerate(observed)])
        prm = ViewParams(w, h, int(cell), int(VIEW_MODES.get(mode, mode)), near, far, float(slack), float(depth_tol))
        return views, cams, prm, obs

    @staticmethod
    def _view_args(clouds, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, want, cam_index):
        """what view refuses before it touches the library, and (View array, Camera array, ViewParams, DeviceImage array or None, points per view)"""
        record = lambda k, c, pose, cam: View(c if isinstance(c, DeviceCloud) else device_cloud(*c, max_n=REDUCE_MAX_POINTS), pose, cam, 0)
        views, cams, prm, obs = CvoReducer._view_call(clouds, "clouds", record, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, want, cam_index)
        return (View * len(views))(*views), cams, prm, obs, [int(v.cloud.n) for v in views]

    def check_view(self, clouds, poses, cameras, size, cell=1, mode="front", slack=0.0, z_range=(0.05, 30.0), observed=None, depth_tol=0.02,
                   cam_index=None):
        """cvo_check_view_clouds on the inputs of `view` with no output arrays (cap 0): the validation alone, nothing is launched"""
        arr, cams, prm, obs, ns = self._view_args(clouds, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, (), cam_index)
        recs = (ViewedCloud * len(ns))()
        _check(self.L.cvo_check_view_clouds(self.h, len(ns), arr, cams, C.byref(prm), obs, recs))

    def view(self, clouds, poses, cameras, size, cell=1, mode="front", slack=0.0, z_range=(0.05, 30.0), observed=None, depth_tol=0.02, cap=65535,
             want=("source",), cam_index=None, stream=None):
        """cvo_view_device_clouds: every posed cloud -- a fused local map -- seen from a camera: the z-buffered subset of its points that the
        camera can see, in input order, by one call.  clouds: a list of what `reduce` takes for one cloud (the same cloud may be listed for
        several views); poses: one 3 x 4 or 4 x 4 array-like per view (host; the cloud's frame to the camera's; the last row of a 4 x 4 is
        ignored); cameras: one (scaling_factor, fx, fy, cx, cy) or a list, with cam_index one index per view; size: (width, height) of the image.
        cell: the side of a z-cell in pixels, 1 .. 16 (voxels.view_cell_for_budget chooses it for a point budget).  mode "front": the nearest
        point of every z-cell alone, at most ceil(w / cell) * ceil(h / cell) rows; "surface": every point within slack (relative) of its
        z-cell's front depth.  z_range: (near, far), points outside are out of view.  observed: one uint16 (h, w) device depth image per view
        (or a (bgr, depth) pair); with it `relation` says per row how the point stands to the measured depth within depth_tol (relative):
        0 unknown, 1 in front (the camera saw through it), 2 agrees, 3 behind, and relation_counts counts the four.  want: which of "source"
        (the input index), "pixel" (py * width + px), "relation", "map" (per input point: its row, -1 hidden, -2 out of view, -3 invalid),
        "depth" and "index" (the z-buffer, (gh, gw): the front's depth and input index, 0 and -1 where empty) to return beside xyz and feat.
        cap, stream: reduce's cap and cloud_stream; the observed images fall under the stream's rule with the clouds: with a stream both must
        have been written on it (or be ordered before it by the caller), with None torch's current stream is synchronised for both and
        anything written on another stream is the caller's to synchronise.  Returns one dict per view; xyz (n_out, 3) is the MOVED position and feat (n_out, 5), and
        they pass into set_pairs_clouds as they are.  Raises CvoError when a view comes to more than cap rows; cap = 0 counts only."""
        import torch
        clouds = list(clouds); observed = None if observed is None else list(observed)
        arr, cams, prm, obs, ns = self._view_args(clouds, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, want, cam_index)
        _settle_cloud_writer(clouds, stream)
        if observed:                                                  # (the depth images' writer too: they may be tensors where the clouds are descriptors)
            _settle_writer([(observed[0][1] if isinstance(observed[0], (tuple, list)) else observed[0], None)], stream)
        n = len(ns)
        gw, gh = -(-prm.width // prm.cell), -(-prm.height // prm.cell)
        most = [min(m, gw * gh) if prm.mode == VIEW_FRONT else m for m in ns]              # (the fronts alone: a row per z-cell at the most)
        caps = [min(int(cap), m) if 0 <= int(cap) <= 65535 else int(cap) for m in most]   # (a cap out of range is the library's to refuse)
        rows = [max(0, c) for c in caps]
        dev = torch.device("cuda", self.device)
        ts = None
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        per_row = dict(xyz=((3,), torch.float32), feat=((5,), torch.float32), source=((), torch.int32), pixel=((), torch.int32), relation=((), torch.int32))
        with torch.cuda.stream(ts):                                   # (the arrays belong to the stream their readers will use)
            whole = {k: torch.empty((sum(rows),) + sh, dtype=dt, device=dev) for k, (sh, dt) in per_row.items() if k in ("xyz", "feat") or k in want}
            mp = torch.empty(sum(ns), dtype=torch.int32, device=dev) if "map" in want else None
            depth = torch.empty((n, gh, gw), dtype=torch.float32, device=dev) if "depth" in want else None
            index = torch.empty((n, gh, gw), dtype=torch.int32, device=dev) if "index" in want else None
        recs = (ViewedCloud * n)(); at = pt = 0; outs = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = {key: t[at:at + rows[k]] for key, t in whole.items()}
            if mp is not None: v["map"] = mp[pt:pt + ns[k]]
            if depth is not None: v["depth"] = depth[k]
            if index is not None: v["index"] = index[k]
            recs[k] = ViewedCloud(*[ptr(v.get(key)) for key in ("xyz", "feat", "source", "pixel", "relation", "map", "depth", "index")], caps[k], 0)
            outs.append(v); at += rows[k]; pt += ns[k]
        n_out = np.zeros(n, np.int32); counts = np.zeros((n, 4), np.int32)
        ip = C.POINTER(C.c_int)
        _check(self.L.cvo_view_device_clouds(self.h, n, arr, cams, C.byref(prm), obs, recs, n_out.ctypes.data_as(ip),
                                             counts.ctypes.data_as(ip) if obs is not None else None, _stream_arg(stream)))
        over = [k for k in range(n) if n_out[k] > caps[k]] if int(cap) != 0 else []      # (cap 0 counts only: n_out is the answer)
        if over:
            k = over[0]
            raise CvoError(CVO_ERR_INVALID, f"view {k}: {int(n_out[k])} rows at cell {prm.cell} are more than cap {int(cap)}: choose a larger cell (view_cell_for_budget)")
        out = []
        whole_cloud = ("map", "depth", "index")
        for k, v in enumerate(outs):
            m = int(n_out[k])
            res = {key: (t if key in whole_cloud else t[:m]) for key, t in v.items()} | dict(n_out=m)
            if obs is not None:
                res["relation_counts"] = counts[k].copy()
            out.append(res)
        return out


# ---- resident maps (cvo_hip.h, "Resident maps"): voxel maps that stay on the device between calls
class CvoMaps:
    """cvo_maps: max_maps independent voxel maps of at most max_rows rows at one voxel size, resident in device memory -- one per tracker
    stream -- to which posed clouds or frames are added (`integrate`) and from which they are taken away again (`remove`), exactly: the sums
    are integers.  Created on a CvoReducer, whose scratch and stream every call uses; close the maps before the reducer.  Every call takes a
    list of map numbers (each at most once) and handles all of them in the same launches.  Outputs are torch tensors on the reducer's device."""

    def __init__(self, reducer: "CvoReducer", max_maps: int, max_rows: int, voxel: float):
        self.L = reducer.L
        self.reducer, self.device = reducer, reducer.device
        self.max_maps, self.max_rows, self.voxel = int(max_maps), int(max_rows), float(voxel)
        self.h = C.c_void_p()
        _check(self.L.cvo_maps_create(reducer.h, self.max_maps, self.max_rows, self.voxel, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.cvo_maps_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """cvo_maps_info: dict(max_maps, max_rows, voxel, device_bytes)"""
        a, b, v, n = C.c_int(0), C.c_int(0), C.c_float(0), C.c_longlong(0)
        _check(self.L.cvo_maps_info(self.h, C.byref(a), C.byref(b), C.byref(v), C.byref(n)))
        return dict(max_maps=a.value, max_rows=b.value, voxel=v.value, device_bytes=n.value)

    def _maps(self, maps):
        """the call's map numbers as an int32 array: all maps for None; refuses an empty list, a number out of range or given twice"""
        ms = list(range(self.max_maps)) if maps is None else [maps] if isinstance(maps, (int, np.integer)) else list(maps)
        if not ms:
            raise ValueError("no maps")
        if any(int(k) != k for k in ms):
            raise ValueError("maps: integers expected")
        ms = [int(k) for k in ms]
        bad = [k for k in ms if not 0 <= k < self.max_maps]
        if bad:
            raise ValueError(f"map {bad[0]}: 0 .. {self.max_maps - 1} expected")
        if len(set(ms)) != len(ms):
            raise ValueError(f"map {[k for k in ms if ms.count(k) > 1][0]} appears twice in the call")
        return np.asarray(ms, np.int32)

    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(C.POINTER(C.c_int))

    def rows(self, maps=None, live: bool = True):
        """cvo_maps_rows: (rows, live_rows) int32 arrays, one entry per listed map: its rows, dead ones included, and those with count >= 1
        (live = False: rows alone, which the host knows: no wait, live_rows is None)"""
        ms = self._maps(maps)
        rows = np.zeros(len(ms), np.int32); alive = np.zeros(len(ms), np.int32) if live else None
        _check(self.L.cvo_maps_rows(self.h, len(ms), self._ip(ms), self._ip(rows), self._ip(alive) if live else None))
        return rows, alive

    def clear(self, maps=None, stream=None):
        """cvo_maps_clear: the listed maps (None: all) become empty"""
        ms = self._maps(maps)
        _check(self.L.cvo_maps_clear(self.h, len(ms), self._ip(ms), _stream_arg(stream)))

    def _stamps(self, ms, groups, stamps):
        """the flat int32 stamps of an update's members: one list of integers >= 0 per group, shaped like groups"""
        if len(groups) != len(ms):
            raise ValueError(f"{len(ms)} maps but {len(groups)} groups")
        stamps = [[q] if isinstance(q, (int, np.integer)) else list(q) for q in stamps]
        if len(stamps) != len(groups):
            raise ValueError(f"{len(groups)} groups but {len(stamps)} lists of stamps")
        flat = []
        for g, (members, st) in enumerate(zip(groups, stamps)):
            if len(st) != len(members):
                raise ValueError(f"group {g}: {len(members)} members but {len(st)} stamps")
            for m, v in enumerate(st):
                if int(v) != v or not 0 <= int(v) < 2 ** 31:
                    raise ValueError(f"group {g} member {m}: stamp {v!r}: an integer in 0 .. 2^31 - 1 expected")
                flat.append(int(v))
        return np.asarray(flat, np.int32)

    def _cloud_update(self, maps, groups, poses, stamps):
        ms = self._maps(maps)
        groups, Ms = CvoReducer._fuse_args(groups, poses, 1, "mean", ())
        st = self._stamps(ms, groups, stamps)
        arr, first, sizes, groups = self.reducer._fuse_inputs(groups, Ms, 1, "mean", ())
        return ms, groups, arr, first, st

    def check_integrate(self, maps, groups, poses, stamps, sign: int = 1):
        """cvo_check_maps_integrate_clouds: the validation of integrate (sign 1) or remove (sign -1) alone, nothing is launched"""
        ms, groups, arr, first, st = self._cloud_update(maps, groups, poses, stamps)
        _check(self.L.cvo_check_maps_integrate_clouds(self.h, len(ms), self._ip(ms), self._ip(first), arr, self._ip(st), int(sign)))

    def _update(self, maps, groups, poses, stamps, sign, cloud_stream):
        ms, groups, arr, first, st = self._cloud_update(maps, groups, poses, stamps)
        _settle_cloud_writer([c for g in groups for c in g], cloud_stream)
        _check(self.L.cvo_maps_integrate_clouds(self.h, len(ms), self._ip(ms), self._ip(first), arr, self._ip(st), sign, _stream_arg(cloud_stream)))

    def integrate(self, maps, groups, poses, stamps, cloud_stream=None):
        """cvo_maps_integrate_clouds, sign +1: group g -- a list of 1 .. 64 posed clouds, what CvoReducer.fuse takes -- is added to map maps[g].
        stamps: a list of lists of integers >= 0 shaped like groups, one per member: the member's bit in view_mask is stamp & 63, and
        last_stamp / born are kept per row.  Raises CvoError, with every map unchanged, when a map would outgrow max_rows or a cell's count
        16777215.  The clouds are read before the call returns."""
        self._update(maps, groups, poses, stamps, 1, cloud_stream)

    def remove(self, maps, groups, poses, stamps, cloud_stream=None, present: bool = False):
        """cvo_maps_integrate_clouds, sign -1: the members go out of their maps again -- the same clouds, poses and stamps that were
        integrated.  Rows whose count reaches 0 are dead until a `compact`.  Raises CvoError, with every map unchanged, when a cell is absent
        or holds fewer members than are taken out.  present = True (sign -2, "remove what is still there"): for maps whose compactions drop
        live rows (drop masks, probation): a cell that is absent, or whose row has none of the members' stamp bits (it was dropped and made
        again by others), is skipped; a row that has some of the bits and not others refuses the call.  After such a compaction plain
        removal is unsupported."""
        self._update(maps, groups, poses, stamps, MAP_REMOVE_PRESENT if present else MAP_REMOVE, cloud_stream)

    def _frame_update(self, maps, groups, poses, stamps, cameras, cam_index, step, swap_rb):
        ms = self._maps(maps)
        groups, Ms = CvoReducer._fuse_args(groups, poses, 1, "mean", ())
        st = self._stamps(ms, groups, stamps)
        flat = [f for g in groups for f in g]
        ci = None if cam_index is None else [int(c) for q in cam_index for c in q]
        descs, w, h, step, cams, ci = CvoReducer._frame_list(flat, cameras, ci, step, swap_rb)
        arr = (FuseFrame * len(descs))(*[FuseFrame(d, (C.c_float * 12)(*M[:3].reshape(-1).tolist()), int(c), 0) for d, M, c in zip(descs, [M for q in Ms for M in q], ci)])
        first = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
        return (self.h, len(ms), self._ip(ms), self._ip(first), arr, w, h, step, cams, self._ip(st)), flat, (ms, first, st, arr, cams)

    def check_integrate_frames(self, maps, groups, poses, stamps, cameras, cam_index=None, step: int = 1, swap_rb=False, sign: int = 1):
        """cvo_check_maps_integrate_frames: the validation of integrate_frames / remove_frames alone"""
        args, flat, keep = self._frame_update(maps, groups, poses, stamps, cameras, cam_index, step, swap_rb)
        _check(self.L.cvo_check_maps_integrate_frames(*args, int(sign)))

    def _update_frames(self, maps, groups, poses, stamps, cameras, cam_index, step, swap_rb, sign, image_stream):
        args, flat, keep = self._frame_update(maps, groups, poses, stamps, cameras, cam_index, step, swap_rb)
        _settle_writer(flat, image_stream)
        _check(self.L.cvo_maps_integrate_frames(*args, sign, _stream_arg(image_stream)))

    def integrate_frames(self, maps, groups, poses, stamps, cameras, cam_index=None, step: int = 1, swap_rb=False, image_stream=None):
        """cvo_maps_integrate_frames, sign +1: `integrate` of the frames' dense clouds (CvoReducer.fuse_frames' members), read in place"""
        self._update_frames(maps, groups, poses, stamps, cameras, cam_index, step, swap_rb, 1, image_stream)

    def remove_frames(self, maps, groups, poses, stamps, cameras, cam_index=None, step: int = 1, swap_rb=False, image_stream=None, present: bool = False):
        """cvo_maps_integrate_frames, sign -1: `remove` of the frames that were integrated (present = True: sign -2, as in `remove`)"""
        self._update_frames(maps, groups, poses, stamps, cameras, cam_index, step, swap_rb, MAP_REMOVE_PRESENT if present else MAP_REMOVE, image_stream)

    @staticmethod
    def _per_map(v, n, name, lo, hi):
        vs = list(v) if hasattr(v, "__len__") else [v] * n
        if len(vs) != n:
            raise ValueError(f"{name}: one value or one per map expected")
        for x in vs:
            if int(x) != x or not lo <= int(x) <= hi:
                raise ValueError(f"{name} {x!r}: an integer in {lo} .. {hi} expected")
        return [int(x) for x in vs]

    def _filters(self, ms, min_points, min_views, min_last_stamp, want):
        bad = [w for w in want if w not in MAP_WANT]
        if bad:
            raise ValueError(f"want: one of {MAP_WANT} expected, got {bad[0]!r}")
        n = len(ms)
        cols = (self._per_map(min_points, n, "min_points", 0, 2 ** 31 - 1), self._per_map(min_views, n, "min_views", 0, FUSE_MAX_MEMBERS),
                self._per_map(min_last_stamp, n, "min_last_stamp", -2 ** 31, 2 ** 31 - 1))
        return (MapFilter * n)(*[MapFilter(a, b, c, 0) for a, b, c in zip(*cols)])

    def check_extract(self, maps=None, min_points=1, min_views=1, min_last_stamp=0):
        """cvo_check_maps_extract with no output arrays (cap 0): the validation alone"""
        ms = self._maps(maps)
        flt = self._filters(ms, min_points, min_views, min_last_stamp, ())
        _check(self.L.cvo_check_maps_extract(self.h, len(ms), self._ip(ms), flt, (MapCloud * len(ms))()))

    def extract(self, maps=None, min_points=1, min_views=1, min_last_stamp=0, cap: int = 65535, want=("count",), stream=None):
        """cvo_maps_extract: the rows of every listed map with count >= max(1, min_points), at least min_views bits in view_mask and
        last_stamp >= min_last_stamp (each one value, or one per map), in ascending row number.  want: which of "count", "views", "view_mask",
        "last_stamp", "born", "row" (the map's row number) to return beside xyz and feat.  Returns one dict per map, as CvoReducer.fuse does:
        xyz (n_out, 3), feat (n_out, 5), the wanted arrays, n_out; the tensors pass into device_cloud / set_pairs_clouds / view as they are.
        Raises CvoError when a map comes to more than cap rows; cap = 0 counts only.  cap is at most 65535 and there is no paging: a
        map may hold up to max_rows rows, but an extract returns its kept rows only when the filter keeps at most 65535 of them."""
        import torch
        ms = self._maps(maps)
        flt = self._filters(ms, min_points, min_views, min_last_stamp, want)
        n = len(ms)
        have, _ = self.rows(ms, live=False)
        caps = [min(int(cap), int(m)) if 0 <= int(cap) <= 65535 else int(cap) for m in have]   # (a cap out of range is the library's to refuse)
        rows = [max(0, c) for c in caps]
        dev = torch.device("cuda", self.device)
        ts = None
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        per_row = dict(xyz=((3,), torch.float32), feat=((5,), torch.float32), count=((), torch.int32), views=((), torch.int32), view_mask=((), torch.int64),
                       last_stamp=((), torch.int32), born=((), torch.int32), row=((), torch.int32))   # (view_mask: 64 bits in torch's signed carrier)
        with torch.cuda.stream(ts):
            whole = {k: torch.empty((sum(rows),) + sh, dtype=dt, device=dev) for k, (sh, dt) in per_row.items() if k in ("xyz", "feat") or k in want}
        recs = (MapCloud * n)(); at = 0; outs = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = {key: t[at:at + rows[k]] for key, t in whole.items()}
            recs[k] = MapCloud(*[ptr(v.get(key)) for key in per_row], caps[k], 0)
            outs.append(v); at += rows[k]
        n_out = np.zeros(n, np.int32)
        _check(self.L.cvo_maps_extract(self.h, n, self._ip(ms), flt, recs, self._ip(n_out), _stream_arg(stream)))
        over = [k for k in range(n) if n_out[k] > caps[k]] if int(cap) != 0 else []
        if over:
            k = over[0]
            raise CvoError(CVO_ERR_INVALID, f"map {int(ms[k])}: {int(n_out[k])} rows are more than cap {int(cap)}: filter harder, compact, or use a larger voxel")
        return [{key: t[:int(n_out[k])] for key, t in v.items()} | dict(n_out=int(n_out[k])) for k, v in enumerate(outs)]

    def _view_records(self, maps, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, min_points, min_views, min_last_stamp, want, carve,
                      cam_index):
        """what view refuses before it touches the library, and (MapView array, Camera array, ViewParams, DeviceImage array or None, map numbers)"""
        ms = [maps] if isinstance(maps, (int, np.integer)) else list(maps)
        if any(int(k) != k for k in ms):
            raise ValueError("maps: integers expected")
        ms = [int(k) for k in ms]
        bad = [k for k in ms if not 0 <= k < self.max_maps]
        if bad:
            raise ValueError(f"map {bad[0]}: 0 .. {self.max_maps - 1} expected")
        if carve and observed is None:
            raise ValueError("carve needs observed")
        n = len(ms)
        cols = (self._per_map(min_points, n, "min_points", 0, 2 ** 31 - 1), self._per_map(min_views, n, "min_views", 0, FUSE_MAX_MEMBERS),
                self._per_map(min_last_stamp, n, "min_last_stamp", -2 ** 31, 2 ** 31 - 1))
        record = lambda k, m, pose, cam: MapView(m, cam, MapFilter(cols[0][k], cols[1][k], cols[2][k], 0), pose)
        views, cams, prm, obs = CvoReducer._view_call(ms, "maps", record, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, want, cam_index)
        return (MapView * n)(*views), cams, prm, obs, ms

    def check_view(self, maps, poses, cameras, size, cell=1, mode="front", slack=0.0, z_range=(0.05, 30.0), observed=None, depth_tol=0.02,
                   min_points=1, min_views=1, min_last_stamp=0, cam_index=None):
        """cvo_check_maps_view on the inputs of `view` with no output arrays (cap 0, no carve): the validation alone, nothing is launched"""
        arr, cams, prm, obs, ms = self._view_records(maps, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, min_points, min_views,
                                                     min_last_stamp, (), False, cam_index)
        _check(self.L.cvo_check_maps_view(self.h, len(ms), arr, cams, C.byref(prm), obs, (ViewedCloud * len(ms))(), None))

    def view(self, maps, poses, cameras, size, cell=1, mode="front", slack=0.0, z_range=(0.05, 30.0), observed=None, depth_tol=0.02, min_points=1,
             min_views=1, min_last_stamp=0, cap=65535, want=("source",), carve=False, cam_index=None, stream=None):
        """cvo_maps_view: every listed map seen from a camera where it lies -- CvoReducer.view of the map's extract, without the extract and
        without its 65535-row ceiling.  maps: one map number per VIEW (a map may be listed for several views: K hypotheses, K filters);
        poses, cameras, cam_index, size, cell, mode, slack, z_range, observed, depth_tol, cap, stream: CvoReducer.view's, the pose taking the
        map's frame to the camera's.  min_points, min_views, min_last_stamp: extract's filter, each one value or one per view.  want: which of
        "source" (the map's row number of each viewed row), "pixel", "relation", "map" (per map row: its viewed row, -1 hidden, -2 out of
        view, -3 invalid, -4 filtered or dead), "depth" and "index" (the z-buffer; index holds map row numbers) to return beside xyz and feat.
        carve = True (needs observed): each dict also has `carve`, a uint8 tensor of the map's rows, 1 where the camera saw through the row
        (visible with relation 1): `compact`'s drop as it is.  Returns one dict per view, as CvoReducer.view does.  Raises CvoError when a view
        comes to more than cap rows; cap = 0 counts only.  The maps are only read."""
        import torch
        observed = None if observed is None else list(observed)
        arr, cams, prm, obs, ms = self._view_records(maps, poses, cameras, size, cell, mode, slack, z_range, observed, depth_tol, min_points, min_views,
                                                     min_last_stamp, want, carve, cam_index)
        if observed:
            _settle_writer([(observed[0][1] if isinstance(observed[0], (tuple, list)) else observed[0], None)], stream)
        n = len(ms)
        uniq = sorted(set(ms))
        have, _ = self.rows(uniq, live=False)
        ns = [int(have[uniq.index(k)]) for k in ms]                    # each view's map rows, dead ones included
        gw, gh = -(-prm.width // prm.cell), -(-prm.height // prm.cell)
        most = [min(m, gw * gh) if prm.mode == VIEW_FRONT else m for m in ns]              # (the fronts alone: a row per z-cell at the most)
        caps = [min(int(cap), m) if 0 <= int(cap) <= 65535 else int(cap) for m in most]   # (a cap out of range is the library's to refuse)
        rows = [max(0, c) for c in caps]
        dev = torch.device("cuda", self.device)
        ts = None
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        per_row = dict(xyz=((3,), torch.float32), feat=((5,), torch.float32), source=((), torch.int32), pixel=((), torch.int32), relation=((), torch.int32))
        with torch.cuda.stream(ts):                                   # (the arrays belong to the stream their readers will use)
            whole = {k: torch.empty((sum(rows),) + sh, dtype=dt, device=dev) for k, (sh, dt) in per_row.items() if k in ("xyz", "feat") or k in want}
            mp = torch.empty(sum(ns), dtype=torch.int32, device=dev) if "map" in want else None
            cv = torch.empty(sum(ns), dtype=torch.uint8, device=dev) if carve else None
            depth = torch.empty((n, gh, gw), dtype=torch.float32, device=dev) if "depth" in want else None
            index = torch.empty((n, gh, gw), dtype=torch.int32, device=dev) if "index" in want else None
        recs = (ViewedCloud * n)(); at = pt = 0; outs = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = {key: t[at:at + rows[k]] for key, t in whole.items()}
            if mp is not None: v["map"] = mp[pt:pt + ns[k]]
            if cv is not None: v["carve"] = cv[pt:pt + ns[k]]
            if depth is not None: v["depth"] = depth[k]
            if index is not None: v["index"] = index[k]
            recs[k] = ViewedCloud(*[ptr(v.get(key)) for key in ("xyz", "feat", "source", "pixel", "relation", "map", "depth", "index")], caps[k], 0)
            outs.append(v); at += rows[k]; pt += ns[k]
        carves = (C.c_void_p * n)(*[ptr(v["carve"]) for v in outs]) if carve else None
        n_out = np.zeros(n, np.int32); counts = np.zeros((n, 4), np.int32)
        _check(self.L.cvo_maps_view(self.h, n, arr, cams, C.byref(prm), obs, recs, carves, self._ip(n_out), self._ip(counts) if obs is not None else None,
                                    _stream_arg(stream)))
        over = [k for k in range(n) if n_out[k] > caps[k]] if int(cap) != 0 else []      # (cap 0 counts only: n_out is the answer)
        if over:
            k = over[0]
            raise CvoError(CVO_ERR_INVALID, f"view {k}: map {ms[k]}: {int(n_out[k])} rows at cell {prm.cell} are more than cap {int(cap)}: choose a larger cell (view_cell_for_budget)")
        out = []
        whole_map = ("map", "carve", "depth", "index")
        for k, v in enumerate(outs):
            m = int(n_out[k])
            res = {key: (t if key in whole_map else t[:m]) for key, t in v.items()} | dict(n_out=m)
            if obs is not None:
                res["relation_counts"] = counts[k].copy()
            out.append(res)
        return out

    # ---- probing maps (cvo_hip.h, "Probing maps"): where a posed member's points fall in a map
    def _probe_records(self, maps, items, what, poses, reach, min_points, min_views, min_last_stamp, want):
        """what a probing call refuses before it touches the library, and (map numbers, MapProbe array, one (C.c_float * 12) pose per probe)"""
        ms = [maps] if isinstance(maps, (int, np.integer)) else list(maps)
        if not ms:
            raise ValueError("no maps")
        if any(int(k) != k for k in ms):
            raise ValueError("maps: integers expected")
        ms = [int(k) for k in ms]
        bad = [k for k in ms if not 0 <= k < self.max_maps]
        if bad:
            raise ValueError(f"map {bad[0]}: 0 .. {self.max_maps - 1} expected")
        bad = [w for w in (want or ()) if w not in PROBE_WANT]
        if bad:
            raise ValueError(f"want: None or some of {PROBE_WANT} expected, got {bad[0]!r}")
        n = len(ms)
        poses = list(poses)
        if len(items) != n:
            raise ValueError(f"{n} maps but {len(items)} {what}")
        if len(poses) != n:
            raise ValueError(f"{n} maps but {len(poses)} poses")
        cols = (self._per_map(reach, n, "reach", 0, 1), self._per_map(min_points, n, "min_points", 0, 2 ** 31 - 1),
                self._per_map(min_views, n, "min_views", 0, FUSE_MAX_MEMBERS), self._per_map(min_last_stamp, n, "min_last_stamp", -2 ** 31, 2 ** 31 - 1))
        Ms = []
        for k, pose in enumerate(poses):
            M = np.asarray(pose, np.float32)
            if M.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"probe {k}: a 3 x 4 or 4 x 4 pose expected, got shape {M.shape}")
            if not np.isfinite(M[:3]).all():
                raise ValueError(f"probe {k}: the pose is not finite")
            Ms.append((C.c_float * 12)(*M[:3].reshape(-1).tolist()))
        return ms, (MapProbe * n)(*[MapProbe(m, r, MapFilter(a, b, c, 0)) for m, r, a, b, c in zip(ms, *cols)]), Ms

    def _cloud_probes(self, maps, clouds, poses, reach, min_points, min_views, min_last_stamp, want):
        clouds = list(clouds)
        ms, prb, Ms = self._probe_records(maps, clouds, "clouds", poses, reach, min_points, min_views, min_last_stamp, want)
        ds = [c if isinstance(c, DeviceCloud) else device_cloud(*c, max_n=REDUCE_MAX_POINTS) for c in clouds]
        return ms, prb, (FuseMember * len(ds))(*[FuseMember(d, M) for d, M in zip(ds, Ms)]), [int(d.n) for d in ds], clouds

    def _frame_probes(self, maps, frames, poses, cameras, cam_index, step, swap_rb, reach, min_points, min_views, min_last_stamp, want):
        frames = list(frames)
        ms, prb, Ms = self._probe_records(maps, frames, "frames", poses, reach, min_points, min_views, min_last_stamp, want)
        descs, w, h, step, cams, ci = CvoReducer._frame_list(frames, cameras, cam_index, step, swap_rb)
        arr = (FuseFrame * len(descs))(*[FuseFrame(d, M, int(c), 0) for d, M, c in zip(descs, Ms, ci)])
        return ms, prb, arr, (w, h, step, cams), [-(-w // step) * -(-h // step)] * len(descs), frames

    def check_probe(self, maps, clouds, poses, reach=0, min_points=1, min_views=1, min_last_stamp=0):
        """cvo_check_maps_probe_clouds on the inputs of `probe` with no output arrays: the validation alone, nothing is launched"""
        ms, prb, arr, ns, clouds = self._cloud_probes(maps, clouds, poses, reach, min_points, min_views, min_last_stamp, None)
        _check(self.L.cvo_check_maps_probe_clouds(self.h, len(ms), prb, arr, (ProbedPoints * len(ms))()))

    def check_probe_frames(self, maps, frames, poses, cameras, cam_index=None, step: int = 1, swap_rb=False, reach=0, min_points=1, min_views=1,
                           min_last_stamp=0):
        """cvo_check_maps_probe_frames on the inputs of `probe_frames` with no output arrays: the validation alone"""
        ms, prb, arr, (w, h, step, cams), ns, frames = self._frame_probes(maps, frames, poses, cameras, cam_index, step, swap_rb, reach, min_points, min_views,
                                                                          min_last_stamp, None)
        _check(self.L.cvo_check_maps_probe_frames(self.h, len(ms), prb, arr, w, h, step, cams, (ProbedPoints * len(ms))()))

    def _run_probe(self, call, ms, ns, want, hit, counts, stream):
        """the output arrays of len(ms) probes of ns points, the call, and the per-probe dicts"""
        import torch
        n = len(ms)
        rows = [0] * n
        if hit:
            uniq = sorted(set(ms))
            have, _ = self.rows(uniq, live=False)
            rows = [int(have[uniq.index(k)]) for k in ms]              # each probe's map rows, dead ones included
        dev = torch.device("cuda", self.device)
        ts = None
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        keys = () if want is None else ("row",) + tuple(k for k in PROBE_WANT if k in want)
        with torch.cuda.stream(ts):                                   # (the arrays belong to the stream their readers will use)
            whole = {k: torch.empty(sum(ns), dtype=torch.float32 if k == "dist2" else torch.int32, device=dev) for k in keys}
            hits = torch.empty(sum(rows), dtype=torch.uint8, device=dev) if hit else None
        recs = (ProbedPoints * n)(); at = ht = 0; outs = []
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        for k in range(n):
            v = {key: t[at:at + ns[k]] for key, t in whole.items()}
            if hits is not None: v["hit"] = hits[ht:ht + rows[k]]
            recs[k] = ProbedPoints(*[ptr(v.get(key)) for key in ("row", "dist2", "count", "views", "last_stamp", "hit")])
            outs.append(v); at += ns[k]; ht += rows[k]
        cnt = np.zeros((n, 4), np.int32) if counts else None
        _check(call(recs, self._ip(cnt) if counts else None))
        return [v | (dict(counts=cnt[k].copy()) if counts else {}) for k, v in enumerate(outs)]

    def probe(self, maps, clouds, poses, reach=0, min_points=1, min_views=1, min_last_stamp=0, want=("dist2",), hit=False, counts=True, cloud_stream=None):
        """cvo_maps_probe_clouds: for every point of a posed cloud, the map row it falls into (reach 0) or lies nearest to among the 27 cells
        around it (reach 1).  maps: one map number per PROBE (a map may be listed for several: K pose hypotheses, K filters); clouds: one of
        what CvoReducer.reduce takes per probe, of any size up to REDUCE_MAX_POINTS; poses: one 3 x 4 or 4 x 4 array-like per probe, the
        cloud's frame to the map's.  reach, min_points, min_views, min_last_stamp (extract's filter): each one value or one per probe.
        Returns one dict per probe: `row` (n,) int32 -- the row number, or -1 absent (no row for the cell, at reach 1 for none of the 27),
        -4 filtered or dead, -3 invalid point -- and of want: "dist2" (float32: the squared distance to the row's mean position, inf where
        row < 0), "count", "views", "last_stamp" (int32: the row's, 0 where row < 0).  hit = True: `hit`, a uint8 tensor of the map's rows,
        1 where some point of the probe has that row.  counts = True: `counts`, numpy int32 (found, absent, filtered, invalid), at the cost
        of the call's one host wait (voxels.probe_shares makes the novelty of them); counts = False with a cloud_stream: no host wait at
        all.  want = None: no per-point arrays, the probe counts only.  The maps are only read."""
        ms, prb, arr, ns, clouds = self._cloud_probes(maps, clouds, poses, reach, min_points, min_views, min_last_stamp, want)
        _settle_cloud_writer(clouds, cloud_stream)
        call = lambda recs, cnt: self.L.cvo_maps_probe_clouds(self.h, len(ms), prb, arr, recs, cnt, _stream_arg(cloud_stream))
        return self._run_probe(call, ms, ns, want, hit, counts, cloud_stream)

    def probe_frames(self, maps, frames, poses, cameras, cam_index=None, step: int = 1, swap_rb=False, reach=0, min_points=1, min_views=1,
                     min_last_stamp=0, want=("dist2",), hit=False, counts=True, image_stream=None):
        """cvo_maps_probe_frames: `probe` of the frames' dense clouds (CvoReducer.dense_frames), read in place.  frames: one (bgr, depth)
        device image per probe, all of one size; cameras: one camera or a list, with cam_index one index per probe; step, swap_rb:
        dense_frames'.  Every array has one entry per sub-grid pixel (voxels.probe_pixels makes the per-pixel image of `row`); a pixel
        without depth is an invalid point."""
        ms, prb, arr, (w, h, step, cams), ns, frames = self._frame_probes(maps, frames, poses, cameras, cam_index, step, swap_rb, reach, min_points, min_views,
                                                                          min_last_stamp, want)
        _settle_writer(frames, image_stream)
        call = lambda recs, cnt: self.L.cvo_maps_probe_frames(self.h, len(ms), prb, arr, w, h, step, cams, recs, cnt, _stream_arg(image_stream))
        return self._run_probe(call, ms, ns, want, hit, counts, image_stream)

    def _compact_args(self, maps, min_last_stamp, min_views, probation_from, drop):
        ms = self._maps(maps)
        n = len(ms)
        cols = (self._per_map(min_last_stamp, n, "min_last_stamp", -2 ** 31, 2 ** 31 - 1), self._per_map(min_views, n, "min_views", 0, FUSE_MAX_MEMBERS),
                self._per_map(probation_from, n, "probation_from", -2 ** 31, 2 ** 31 - 1))
        keep = (MapKeep * n)(*[MapKeep(a, b, c, 0) for a, b, c in zip(*cols)])
        drops = None
        if drop is not None:
            drop = list(drop)
            if len(drop) != n:
                raise ValueError(f"{n} maps but {len(drop)} drop masks")
            ptrs = []
            for k, d in enumerate(drop):
                if d is None:
                    ptrs.append(None); continue
                cai = getattr(d, "__cuda_array_interface__", None)
                if cai is None:
                    raise ValueError(f"drop {k}: a device array (__cuda_array_interface__) expected")
                if cai["typestr"] not in ("|u1", "|b1", "|i1") or len(cai["shape"]) != 1 or cai.get("strides") not in (None, (1,)):
                    raise ValueError(f"drop {k}: a contiguous 1-D array of bytes (uint8 or bool) expected")
                ptrs.append(cai["data"][0] if cai["shape"][0] else None)
            drops = (C.c_void_p * n)(*ptrs)
        return ms, keep, drop, drops

    def check_compact(self, maps=None, min_last_stamp=0, min_views=0, probation_from=0, drop=None):
        """cvo_check_maps_compact: the validation alone"""
        ms, keep, drop, drops = self._compact_args(maps, min_last_stamp, min_views, probation_from, drop)
        _check(self.L.cvo_check_maps_compact(self.h, len(ms), self._ip(ms), keep, drops, None))

    def compact(self, maps=None, min_last_stamp=0, min_views=0, probation_from=0, drop=None, new_row: bool = False, stream=None):
        """cvo_maps_compact: in every listed map a row stays when count >= 1, last_stamp >= min_last_stamp, (its views >= min_views or
        born >= probation_from), and its byte in drop[k] is 0 (drop: None, or one 1-D uint8 / bool device array of the map's rows, or None,
        per map; voxels.carve_mask makes one from a view).  The survivors keep their order and are renumbered from 0.  The defaults drop the
        dead rows alone.  Returns the new row counts (int32 array), and with new_row also a list of int32 tensors: each old row's new number
        or -1."""
        import torch
        ms, keep, drop, drops = self._compact_args(maps, min_last_stamp, min_views, probation_from, drop)
        n = len(ms)
        have, _ = self.rows(ms, live=False)
        if drop is not None:
            for k, d in enumerate(drop):
                if d is not None and int(d.__cuda_array_interface__["shape"][0]) != int(have[k]):
                    raise ValueError(f"drop {k}: {int(d.__cuda_array_interface__['shape'][0])} bytes for map {int(ms[k])}'s {int(have[k])} rows")
        news = ptrs = None
        if new_row:
            dev = torch.device("cuda", self.device)
            ts = None
            if stream is not None:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
            with torch.cuda.stream(ts):
                news = [torch.empty(int(m), dtype=torch.int32, device=dev) for m in have]
            ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in news])
        out = np.zeros(n, np.int32)
        if stream is None and drop is not None and "torch" in sys.modules:
            sys.modules["torch"].cuda.current_stream(self.device).synchronize()          # (the masks' writer: torch's current stream)
        _check(self.L.cvo_maps_compact(self.h, n, self._ip(ms), keep, drops, ptrs, self._ip(out), _stream_arg(stream)))
        return (out, news) if new_row else out

    # -- saving and restoring (cvo_hip.h, "Saving and restoring maps")
    @staticmethod
    def _device_array(a):
        """(pointer, shape, item bytes, kind letter, contiguous) of a device array, or None when `a` is none.  A torch tensor is asked
        directly: its __cuda_array_interface__ costs microseconds a look, and a call over 64 maps looks at 384 arrays."""
        if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):
            if not a.is_cuda:
                return None
            name = str(a.dtype)
            kind = "f" if a.is_floating_point() or a.is_complex() else "b" if name == "torch.bool" else "u" if name.startswith("torch.uint") else "i"
            return a.data_ptr(), tuple(int(v) for v in a.shape), a.element_size(), kind, a.is_contiguous()
        cai = getattr(a, "__cuda_array_interface__", None)
        if cai is None:
            return None
        shape = tuple(int(v) for v in cai["shape"])
        ts = cai["typestr"]
        item = int(ts[2:])
        dense = tuple(item * int(np.prod(shape[j + 1:])) for j in range(len(shape)))
        return cai["data"][0], shape, item, ts[1] if ts[0] in "<|=" else "?", cai.get("strides") in (None, dense)

    def _snap_records(self, ms, snaps, what):
        """what a snapshot or a restore refuses before it touches the library, and the MapSnapshot array: one dict per map with the six device
        arrays (anything with __cuda_array_interface__) and optionally `rows` (default: the arrays' length)"""
        snaps = [snaps] if isinstance(snaps, dict) else list(snaps)
        if len(snaps) != len(ms):
            raise ValueError(f"{len(ms)} maps but {len(snaps)} snapshots")
        recs = (MapSnapshot * len(ms))()
        for k, sn in enumerate(snaps):
            if not isinstance(sn, dict):
                raise ValueError(f"{what} {k}: a dict of device arrays expected")
            ptrs, lens = [], []
            for name, size, kinds, tail in SNAPSHOT_FIELDS:
                a = sn.get(name)
                if a is None:
                    ptrs.append(None); lens.append(None); continue
                info = self._device_array(a)
                if info is None:
                    raise ValueError(f"{what} {k}: {name}: a device array (__cuda_array_interface__) expected")
                ptr, shape, item, kind, contiguous = info
                if kind not in kinds or item != size or shape[1:] != tail or len(shape) != 1 + len(tail) or not contiguous:
                    raise ValueError(f"{what} {k}: {name}: a contiguous {size}-byte integer array of shape (rows{', 8' if tail else ''}) expected, got {kind}{item} {shape}")
                ptrs.append(ptr if shape[0] else None); lens.append(shape[0])
            have = [v for v in lens if v is not None]
            rows = sn.get("rows", min(have) if have else 0)
            if int(rows) != rows or not 0 <= int(rows) < 2 ** 31:
                raise ValueError(f"{what} {k}: rows {rows!r}: an integer in 0 .. 2^31 - 1 expected")
            rows = int(rows)
            for (name, _, _, _), n in zip(SNAPSHOT_FIELDS, lens):
                if (n is None and rows > 0) or (n is not None and n < rows):
                    raise ValueError(f"{what} {k}: {name} has {0 if n is None else n} rows, below rows {rows}")
            recs[k] = MapSnapshot(*ptrs, rows, 0)
        return recs, snaps

    def empty_snapshots(self, rows, stream=None):
        """one dict of uninitialised device tensors per entry of `rows`, each with room for that many rows: what snapshot_into fills"""
        import torch
        dev = torch.device("cuda", self.device)
        ts = None
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        kinds = dict(keys=torch.int64, sums=torch.int64, count=torch.int32, view_mask=torch.int64, last_stamp=torch.int32, born=torch.int32)
        with torch.cuda.stream(ts):                                    # (keys, count, view_mask: unsigned bits in torch's signed carriers)
            return [{name: torch.empty((int(n),) + tail, dtype=kinds[name], device=dev) for name, _, _, tail in SNAPSHOT_FIELDS} | dict(rows=int(n)) for n in rows]

    def check_snapshot(self, maps, snaps):
        """cvo_check_maps_snapshot on what snapshot_into takes: the validation alone, nothing is launched"""
        ms = self._maps(maps)
        recs, snaps = self._snap_records(ms, snaps, "snapshot")
        _check(self.L.cvo_check_maps_snapshot(self.h, len(ms), self._ip(ms), recs))

    def snapshot_into(self, maps, snaps, stream=None):
        """cvo_maps_snapshot into arrays the caller has: snaps[k]'s six device arrays (empty_snapshots' dicts; `rows`: their capacity) take map
        maps[k]'s rows 0 .. rows - 1 as they stand, dead ones included; nothing behind them is touched.  A capacity below a map's rows refuses
        the call.  Returns the maps' row counts (int32 array).  With a stream there is no host wait."""
        ms = self._maps(maps)
        recs, snaps = self._snap_records(ms, snaps, "snapshot")
        out = np.zeros(len(ms), np.int32)
        _check(self.L.cvo_maps_snapshot(self.h, len(ms), self._ip(ms), recs, self._ip(out), _stream_arg(stream)))
        return out

    def snapshot(self, maps=None, stream=None):
        """cvo_maps_snapshot: the rows of every listed map (None: all) as they stand, dead ones included.  Returns one dict per map of device
        tensors with one entry per row -- keys (int64 carrier of the 64 bits), sums (rows, 8) int64, count (int32 carrier), view_mask (int64
        carrier), last_stamp, born (int32) -- and rows.  `restore` on any CvoMaps of the same voxel makes the same map of them; voxels.save_maps
        writes them to a file.  The maps are only read; with a stream there is no host wait."""
        ms = self._maps(maps)
        have, _ = self.rows(ms, live=False)
        snaps = self.empty_snapshots(have, stream)
        self.snapshot_into(ms, snaps, stream)
        return snaps

    def check_restore(self, maps, snaps, voxel=None):
        """cvo_check_maps_restore: the validation of `restore` alone, nothing is launched"""
        ms = self._maps(maps)
        recs, snaps = self._snap_records(ms, snaps, "snapshot")
        _check(self.L.cvo_check_maps_restore(self.h, len(ms), self._ip(ms), recs, self.voxel if voxel is None else float(voxel)))

    def restore(self, maps, snaps, voxel=None, stream=None):
        """cvo_maps_restore: map maps[k] becomes exactly the rows of snaps[k] (a `snapshot`'s dict, or any six device arrays of that layout with
        `rows`, default their length); what it held before is gone.  voxel: the size the keys were made at (None: this object's); it must have
        the bits of this object's voxel.  The rows are untrusted: each is tested on the device first, and a bad key (bit 1), a count above
        16777215 (2), a negative stamp (4), a sum out of bound (8) or a duplicate key (16) raises CvoError naming the map and its bits, with
        every listed map unchanged.  stream None: the arrays are taken as written on torch's current stream."""
        ms = self._maps(maps)
        recs, snaps = self._snap_records(ms, snaps, "snapshot")
        if stream is None and "torch" in sys.modules:
            sys.modules["torch"].cuda.current_stream(self.device).synchronize()          # (the arrays' writer: torch's current stream)
        _check(self.L.cvo_maps_restore(self.h, len(ms), self._ip(ms), recs, self.voxel if voxel is None else float(voxel), _stream_arg(stream)))

    def grown(self, max_rows: int):
        """A new CvoMaps on the same reducer with max_rows rows per map and every map restored from this one: the remedy for a map that an
        integration would take above max_rows.  This object stays as it is; close it when the new one has taken over."""
        new = CvoMaps(self.reducer, self.max_maps, int(max_rows), self.voxel)
        try:
            new.restore(None, self.snapshot(None))
        except Exception:
            new.close()
            raise
        return new

    # -- merging (cvo_hip.h, "Merging maps")
    def _merge_records(self, dst_maps, src, src_maps, level, all_rows, min_points, min_views, min_last_stamp):
        """what a merge refuses before it touches the library, and the MapMerge array: this object is the destination"""
        if not isinstance(src, CvoMaps):
            raise ValueError("src: a CvoMaps expected")
        if int(level) != level or not 0 <= int(level) <= MAP_MERGE_MAX_LEVEL:
            raise ValueError(f"level {level!r}: an integer in 0 .. {MAP_MERGE_MAX_LEVEL} expected")
        ds = self._maps(dst_maps)                                      # (each destination at most once)
        ss = [src_maps] if isinstance(src_maps, (int, np.integer)) else list(range(src.max_maps)) if src_maps is None else list(src_maps)
        if len(ss) != len(ds):
            raise ValueError(f"{len(ds)} destination maps but {len(ss)} source maps")
        if any(int(k) != k for k in ss):
            raise ValueError("src_maps: integers expected")
        ss = [int(k) for k in ss]                                      # (a source may stand in several merges)
        bad = [k for k in ss if not 0 <= k < src.max_maps]
        if bad:
            raise ValueError(f"source map {bad[0]}: 0 .. {src.max_maps - 1} expected")
        if src is self:
            both = [k for k in ss if k in set(ds.tolist())]
            if both:
                raise ValueError(f"map {both[0]} is both a source and a destination of the call")
        n = len(ds)
        flt = self._filters(ds, min_points, min_views, min_last_stamp, ())
        every = [all_rows] * n if isinstance(all_rows, (bool, int, np.integer)) else list(all_rows)
        if len(every) != n:
            raise ValueError("all_rows: one value or one per merge expected")
        return (MapMerge * n)(*[MapMerge(int(d), s, 1 if a else 0, 0, f) for d, s, a, f in zip(ds, ss, every, flt)]), n

    def check_merge(self, dst_maps, src, src_maps, level=0, all_rows=True, min_points=1, min_views=0, min_last_stamp=0):
        """cvo_check_maps_merge: the validation of `merge` alone, nothing is launched"""
        recs, n = self._merge_records(dst_maps, src, src_maps, level, all_rows, min_points, min_views, min_last_stamp)
        _check(self.L.cvo_check_maps_merge(self.h, n, recs, src.h, int(level)))

    def merge(self, dst_maps, src, src_maps, level=0, all_rows=True, min_points=1, min_views=0, min_last_stamp=0, stream=None):
        """cvo_maps_merge: the kept rows of map src_maps[k] of `src` (a CvoMaps on this device; it may be this object) are added into this
        object's map dst_maps[k], each into the cell that its own cell shifts to at this object's voxel, which must be ldexp(src.voxel,
        level) bit for bit (level 0: the same voxel, a union).  all_rows (one value or one per merge): every row, dead ones included -- then
        the result is, in every field but born, the map the source's own history would have built at this voxel; otherwise the rows that
        extract's filter (min_points, min_views, min_last_stamp: one value or one per merge) keeps.  A destination stands at most once, a
        source may stand in several merges.  Raises CvoError, with every map unchanged, when a destination would outgrow max_rows or a cell's
        count 16777215, or when a source has more rows than this object's reducer's max_points.  Runs on this object's reducer's stream;
        when src is on another reducer, its writes must be done."""
        recs, n = self._merge_records(dst_maps, src, src_maps, level, all_rows, min_points, min_views, min_last_stamp)
        _check(self.L.cvo_maps_merge(self.h, n, recs, src.h, int(level), _stream_arg(stream)))

    def coarser(self, level: int, max_rows=None):
        """A new CvoMaps on the same reducer at ldexp(voxel, level) with every map merged from this one with all rows: the whole map at a
        voxel 2^level times as large, for an extract under the align kernel's point budget.  max_rows: None for this object's.  This
        object stays as it is."""
        if int(level) != level or not 0 <= int(level) <= MAP_MERGE_MAX_LEVEL:
            raise ValueError(f"level {level!r}: an integer in 0 .. {MAP_MERGE_MAX_LEVEL} expected")
        from .voxels import coarser_voxel
        new = CvoMaps(self.reducer, self.max_maps, self.max_rows if max_rows is None else int(max_rows), coarser_voxel(self.voxel, int(level)))
        try:
            new.merge(None, self, None, level=int(level))
        except Exception:
            new.close()
            raise
        return new


# ---- per-point support and point matches (cvo_hip.h, "per-point support", "point matches"): the output records of all their forms.
# A kind: its C record, its array keys (name, typestr, width), whether the record carries `fit`.
_MATCH_FIELDS = (("best", "<i4", 1), ("best_value", "<f4", 1), ("mean", "<f4", 3), ("sum", "<f4", 1), ("count", "<i4", 1))
_MATCH_KEYS = tuple((f"{name}_{side}", typestr, width) for side in ("moving", "fixed") for name, typestr, width in _MATCH_FIELDS)
_SUPPORT_KEYS = tuple(k for k in _MATCH_KEYS if k[0].startswith(("sum", "count")))
_MATCH_FIT_DTYPE = np.dtype([("rows", "<i4"), ("matched", "<i4"), ("sum_w", "<f8"), ("sum_w_res2", "<f8")])     # cvo_match_fit
_SUPPORT = (PointSupportDst, _SUPPORT_KEYS, False)
_MATCHES = (PointMatchesDst, _MATCH_KEYS, True)


def _host_records(kind, sizes):
    """numpy arrays for pairs of (n_moving, n_fixed) points under the kind's keys, their fit records (None where the kind has none), and the C
    records that point at them"""
    Dst, keys, with_fit = kind
    arrays, fits = [], np.zeros((max(1, len(sizes)), 2), _MATCH_FIT_DTYPE) if with_fit else None
    recs = (Dst * max(1, len(sizes)))()
    for k, (r, (nm, nf)) in enumerate(zip(recs, sizes)):
        a = {}
        for key, typestr, width in keys:
            n = nm if key.endswith("moving") else nf
            a[key] = np.zeros(n if width == 1 else (n, width), np.dtype(typestr))
            setattr(r, key, a[key].ctypes.data)
        if with_fit:
            r.fit = fits[k].ctypes.data
        arrays.append(a)
    return arrays, fits, recs


def _device_records(kind, out, sizes):
    """records over caller-owned device arrays: out[k] is a dict with a direction's arrays under the kind's keys (support: sum_*, count_*; matches:
    best_*, best_value_*, mean_* (n, 3), sum_*, count_*; a direction may be left out) and, for matches, optionally `fit`, 48 bytes of device
    memory for the two fit records (six float64 or 48 uint8; read it back with match_fit_records) -- each anything with
    __cuda_array_interface__ (torch ROCm tensors), contiguous, one row per point of its cloud"""
    Dst, keys, with_fit = kind
    if len(out) != len(sizes):
        raise ValueError("out: one dict per pair")
    recs = (Dst * max(1, len(out)))()
    if with_fit:
        keys = keys + (("fit", None, 0),)
    known = {k for k, _, _ in keys}
    for r, o, (nm, nf) in zip(recs, out, sizes):
        if set(o) - known:
            raise ValueError(f"out: unknown keys {sorted(set(o) - known)}")
        for key, typestr, width in keys:
            a = o.get(key)
            if a is None:
                continue
            if not hasattr(a, "__cuda_array_interface__"):
                raise ValueError(f"out[{key}]: device memory wanted, an object with __cuda_array_interface__ (host arrays: out=None)")
            cai = a.__cuda_array_interface__
            shape, item = tuple(cai["shape"]), int(cai["typestr"][2:])
            if key == "fit":
                if len(shape) != 1 or shape[0] * item != 48:
                    raise ValueError(f"out[fit]: shape {shape} of {cai['typestr']}, wanted 48 bytes in one dimension")
                want_strides = (item,)
            else:
                n = nm if key.endswith("moving") else nf
                if cai["typestr"] != typestr:
                    raise ValueError(f"out[{key}]: dtype {cai['typestr']}, wanted {typestr}")
                if shape != ((n,) if width == 1 else (n, width)):
                    raise ValueError(f"out[{key}]: shape {shape}, the cloud has {n} points")
                want_strides = (4,) if width == 1 else (4 * width, 4)
            if cai.get("strides") not in (None, want_strides):
                raise ValueError(f"out[{key}]: not contiguous")
            setattr(r, key, int(cai["data"][0]))
    return recs


def _settle_support_writer(out, out_stream):
    """out_stream None: the arrays are taken as ready to be written.  torch tensors are touched on torch's current stream, so that stream is
    synchronised first (as _settle_writer does for images that are read)."""
    if out_stream is not None or "torch" not in sys.modules or not out:
        return
    torch = sys.modules["torch"]
    for a in out[0].values():
        if isinstance(a, torch.Tensor) and a.is_cuda:
            torch.cuda.current_stream(a.device).synchronize()
            return


def match_fit_records(raw):
    """(fit_moving, fit_fixed) as dicts out of the 48 bytes of a point-matches `fit` array (a host copy of the device form's)"""
    rec = np.frombuffer(np.ascontiguousarray(raw).tobytes(), _MATCH_FIT_DTYPE, count=2)
    return tuple({k: (int(r[k]) if k in ("rows", "matched") else float(r[k])) for k in _MATCH_FIT_DTYPE.names} for r in rec)


def _match_host_results(arrays, fits):
    for k, a in enumerate(arrays):
        a["fit_moving"], a["fit_fixed"] = match_fit_records(fits[k])
    return arrays


class Cvo:
    """One `cvo::cvo` object (cvo.hpp:82-282) living on a gfx950 device."""

    def __init__(self, params: Params | None = None, device: int = 0):
        self.L = load_library()
        self.params = params or default_params()
        self.h = C.c_void_p()
        _check(self.L.cvo_create(C.byref(self.params), device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.cvo_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- cvo.cpp:345-386 (cloud handed in instead of RGB/depth)
    def set_pcd(self, xyz, feat):
        x, xp, f, fpt = _cloud_args(xyz, feat)
        _check(self.L.cvo_set_pcd(self.h, xp, fpt, x.shape[0]))

    # -- cvo.cpp:345-386 with the images, as the reference's signature has it (pcd_generator on the GPU)
    @staticmethod
    def _images(bgr8, depth16):
        bgr = np.ascontiguousarray(bgr8, np.uint8); dep = np.ascontiguousarray(depth16, np.uint16)
        h, w = dep.shape
        if bgr.shape != (h, w, 3):
            raise ValueError("bgr8 must be (h, w, 3) for a (h, w) depth image")
        return bgr, dep, w, h

    def set_pcd_images(self, bgr8, depth16, camera):
        """camera = (scaling_factor, fx, fy, cx, cy)."""
        bgr, dep, w, h = self._images(bgr8, depth16); cam = Camera(*[float(v) for v in camera])
        _check(self.L.cvo_set_pcd_images(self.h, bgr.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p), w, h, C.byref(cam)))

    def stage_next_frame(self, bgr8, depth16, camera):
        """cvo_stage_next_frame: start generating this frame's cloud now; a later set_pcd_images / match_*_images with the same images takes it.
        The arrays are kept alive (and must not be written) until then."""
        bgr, dep, w, h = self._images(bgr8, depth16); cam = Camera(*[float(v) for v in camera])
        self._staged = (bgr, dep)                                    # the library reads them from its worker thread
        _check(self.L.cvo_stage_next_frame(self.h, bgr.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p), w, h, C.byref(cam)))

    def staged_frame_count(self) -> int:
        """cvo_staged_frame_count: clouds this object took from a generation started ahead of time"""
        n = C.c_int(0); _check(self.L.cvo_staged_frame_count(self.h, C.byref(n))); return n.value

    def set_num_want(self, num_want: int):
        _check(self.L.cvo_set_num_want(self.h, int(num_want)))

    def match_keyframe_images(self, bgr8, depth16, camera):
        bgr, dep, w, h = self._images(bgr8, depth16); cam = Camera(*[float(v) for v in camera]); out = np.zeros(12, np.float64)
        _check(self.L.cvo_match_keyframe_images(self.h, bgr.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p), w, h, C.byref(cam),
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 4)

    def match_odometry_images(self, bgr8, depth16, camera):
        bgr, dep, w, h = self._images(bgr8, depth16); cam = Camera(*[float(v) for v in camera]); out = np.zeros(12, np.float64)
        _check(self.L.cvo_match_odometry_images(self.h, bgr.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p), w, h, C.byref(cam),
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 4)

    def get_cloud(self, slot: int):
        n = C.c_int(0)
        _check(self.L.cvo_get_cloud(self.h, slot, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32); feat = np.zeros((5, n.value), np.float32)
        if n.value:
            _check(self.L.cvo_get_cloud(self.h, slot, xyz.ctypes.data_as(C.POINTER(C.c_float)), feat.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return xyz, feat

    def get_selected_points(self, slot: int):
        n = C.c_int(0)
        _check(self.L.cvo_get_selected_points(self.h, slot, None, 0, C.byref(n)))
        px = np.zeros((n.value, 2), np.uint16)
        if n.value:
            _check(self.L.cvo_get_selected_points(self.h, slot, px.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return px

    # -- cvo.cpp:763-821
    def align(self, trace_cap: int = 0):
        if trace_cap:
            rows = (TraceRow * trace_cap)(); n = C.c_int(0)
            _check(self.L.cvo_align_traced(self.h, rows, trace_cap, C.byref(n)))
            return [dict(omega=np.array(r.omega[:], np.float32), v=np.array(r.v[:], np.float32), nnz=r.nnz,
                         candidates=r.candidates, BCDE=np.array([r.B, r.C, r.D, r.E]), step=r.step, ell=r.ell, dist=r.dist)
                    for r in rows[: min(n.value, trace_cap)]]
        _check(self.L.cvo_align(self.h))
        return None

    # -- cvo.cpp:461-473 / 563-576.  "cvo not initialized !" -> CvoError(code 1), output untouched
    def match_odometry(self, xyz, feat):
        x, xp, f, fpt = _cloud_args(xyz, feat); out = np.zeros(12, np.float64)
        _check(self.L.cvo_match_odometry(self.h, xp, fpt, x.shape[0], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 4)

    def match_keyframe(self, xyz, feat):
        x, xp, f, fpt = _cloud_args(xyz, feat); out = np.zeros(12, np.float64)
        _check(self.L.cvo_match_keyframe(self.h, xp, fpt, x.shape[0], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 4)

    # -- cvo.cpp:388-459
    def function_inner_product(self, slot_a, tran_a, slot_b):
        r = InnP(); t, tp = _tran(tran_a)
        _check(self.L.cvo_function_inner_product(self.h, slot_a, tp, slot_b, C.byref(r)))
        return (r.value, r.num, r.num_e)

    # -- not in the reference: the terms of function_inner_product per point (cvo_hip.h, "per-point support")
    def point_support(self, slot_a, tran_a, slot_b):
        """(sum_a, count_a, sum_b, count_b): per point of the cloud in slot_a (moved by tran_a when given) the sum and number of its kernel
        values against slot_b's points inside both gates, and the same per point of slot_b"""
        na, nb = C.c_int(0), C.c_int(0)
        _check(self.L.cvo_get_cloud(self.h, slot_a, None, None, 0, C.byref(na))); _check(self.L.cvo_get_cloud(self.h, slot_b, None, None, 0, C.byref(nb)))
        sa = np.zeros(na.value, np.float32); ca = np.zeros(na.value, np.int32); sb = np.zeros(nb.value, np.float32); cb = np.zeros(nb.value, np.int32)
        fp = C.POINTER(C.c_float); ip = C.POINTER(C.c_int); t, tp = _tran(tran_a)
        _check(self.L.cvo_point_support(self.h, slot_a, tp, slot_b, sa.ctypes.data_as(fp), ca.ctypes.data_as(ip), na.value,
                                        sb.ctypes.data_as(fp), cb.ctypes.data_as(ip), nb.value))
        return sa, ca, sb, cb

    # -- not in the reference: what each point was matched to (cvo_hip.h, "point matches")
    def point_matches(self, slot_a, tran_a, slot_b):
        """A dict: per point of the cloud in slot_a (moved by tran_a when given; keys *_moving) and per point of slot_b's (*_fixed) the index of its
        best partner in the other cloud (best, -1: none), that kernel value (best_value), the kernel-weighted mean of its partners' points in
        slot_b's frame (mean, (n, 3)) and point_support's sum and count; fit_moving / fit_fixed: the directions' fit records as dicts
        (cvo_slam_amd.matches: fitness, rmse, mutual, residuals)."""
        na, nb = C.c_int(0), C.c_int(0)
        _check(self.L.cvo_get_cloud(self.h, slot_a, None, None, 0, C.byref(na))); _check(self.L.cvo_get_cloud(self.h, slot_b, None, None, 0, C.byref(nb)))
        arrays, fits, recs = _host_records(_MATCHES, [(na.value, nb.value)])
        t, tp = _tran(tran_a)
        _check(self.L.cvo_point_matches(self.h, slot_a, tp, slot_b, recs, na.value, nb.value))
        return _match_host_results(arrays, fits)[0]

    # -- not in the reference: K start transforms scored before an alignment (cvo_hip.h, "pose hypotheses")
    def score_hypotheses(self, slot_a, slot_b, trans, ell=None):
        """(values float32[K], nums int32[K], best): function_inner_product of slot_a's cloud under each of the K transforms `trans` (K x 3 x 4, moving ->
        fixed) against slot_b's cloud at length scale ell (None: params.ell), in one launch; best = the lowest index of the largest value.  The object's
        state is untouched."""
        t, k = _hyp_trans(np.asarray(trans, np.float32).reshape(1, -1, 12), 1)
        recs = (InnP * max(k, 1))(); best = C.c_int(-1)
        _check(self.L.cvo_score_hypotheses(self.h, int(slot_a), int(slot_b), k, t.ctypes.data_as(C.POINTER(C.c_float)),
                                           float(self.params.ell if ell is None else ell), recs, C.byref(best)))
        v, n = _inn_arrays(recs, (k,))
        return v, n, int(best.value)

    # -- not in the reference: how the inner product changes with the pose (cvo_hip.h, "pose models")
    def pose_models(self, slot_a, slot_b, trans, ell=None):
        """(values float32[K], nums int32[K], grads float64[K, 6], hess float64[K, 6, 6]): value, se(3) gradient and Hessian (twist [omega; v] in the
        fixed frame, applied on the left) of function_inner_product of slot_a's cloud under each of the K transforms `trans` against slot_b's cloud at
        length scale ell (None: params.ell), in one launch.  The object's state is untouched."""
        t, k = _hyp_trans(np.asarray(trans, np.float32).reshape(1, -1, 12), 1)
        recs = (PoseModel * max(k, 1))()
        _check(self.L.cvo_pose_models(self.h, int(slot_a), int(slot_b), k, t.ctypes.data_as(C.POINTER(C.c_float)),
                                      float(self.params.ell if ell is None else ell), recs))
        return _model_arrays(recs, (k,))

    # -- cvo.cpp:620-759
    def se3_hessian(self, slot_a, tran_a, slot_b, inliers: int = 0):
        H = np.zeros(36); inl = C.c_int(inliers); t, tp = _tran(tran_a)
        _check(self.L.cvo_se3_hessian(self.h, slot_a, tp, slot_b, H.ctypes.data_as(C.POINTER(C.c_double)), C.byref(inl)))
        return H.reshape(6, 6), inl.value

    # -- the same two on clouds handed in directly, as the reference's members take them (cvo.hpp:222, 260)
    def function_inner_product_clouds(self, xyz_a, feat_a, xyz_b, feat_b):
        a, ap, fa, fap = _cloud_args(xyz_a, feat_a); b, bp, fb, fbp = _cloud_args(xyz_b, feat_b); r = InnP()
        _check(self.L.cvo_function_inner_product_clouds(self.h, ap, fap, a.shape[0], bp, fbp, b.shape[0], C.byref(r)))
        return (r.value, r.num, r.num_e)

    def se3_hessian_clouds(self, xyz_a, feat_a, xyz_b, feat_b, inliers: int = 0):
        a, ap, fa, fap = _cloud_args(xyz_a, feat_a); b, bp, fb, fbp = _cloud_args(xyz_b, feat_b)
        H = np.zeros(36); inl = C.c_int(inliers)
        _check(self.L.cvo_se3_hessian_clouds(self.h, ap, fap, a.shape[0], bp, fbp, b.shape[0], H.ctypes.data_as(C.POINTER(C.c_double)), C.byref(inl)))
        return H.reshape(6, 6), inl.value

    # -- cvo.cpp:475-503
    def compute_innerproduct(self, tran):
        pre, post, fx, mv = InnP(), InnP(), InnP(), InnP()
        H = np.zeros(36); inl = C.c_int(0); cos = C.c_float(0); t, tp = _tran(tran)
        _check(self.L.cvo_compute_innerproduct(self.h, C.byref(pre), C.byref(post), H.ctypes.data_as(C.POINTER(C.c_double)), tp,
                                               C.byref(inl), C.byref(fx), C.byref(mv), C.byref(cos)))
        tup = lambda r: (r.value, r.num, r.num_e)
        return dict(inn_pre=tup(pre), inn_post=tup(post), post_hessian=H.reshape(6, 6), inliers=inl.value,
                    inn_fixed_pcd=tup(fx), inn_moving_pcd=tup(mv), cos_angle=cos.value)

    # -- cvo.cpp:505-561
    def compute_innerproduct_lc(self, prior_tran, lc_prior_tran, lc_prior_tran_2, lc_tran):
        prior, lcp, lcpre, lcpost, fx, mv = (InnP() for _ in range(6))
        H = np.zeros(36); i1 = C.c_int(0); i2 = C.c_int(0); cos = C.c_float(0)
        keep = [_tran(t) for t in (prior_tran, lc_prior_tran, lc_prior_tran_2, lc_tran)]
        _check(self.L.cvo_compute_innerproduct_lc(self.h, C.byref(prior), C.byref(lcp), C.byref(lcpre), C.byref(lcpost),
                                                  H.ctypes.data_as(C.POINTER(C.c_double)), keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                                  C.byref(i1), C.byref(i2), C.byref(fx), C.byref(mv), C.byref(cos)))
        tup = lambda r: (r.value, r.num, r.num_e)
        return dict(inn_prior=tup(prior), inn_lc_prior=tup(lcp), inn_lc_pre=tup(lcpre), inn_lc_post=tup(lcpost),
                    post_hessian=H.reshape(6, 6), inliers_svd=i1.value, inliers_pnpransac=i2.value,
                    inn_fixed_pcd=tup(fx), inn_moving_pcd=tup(mv), cos_angle=cos.value)

    # -- cvo.cpp:578-618
    def update_fixed_pcd(self): _check(self.L.cvo_update_fixed_pcd(self.h))
    def update_previous_pcd(self): _check(self.L.cvo_update_previous_pcd(self.h))

    def reset_keyframe(self, odometry):
        t, tp = _tran(odometry); _check(self.L.cvo_reset_keyframe(self.h, tp))

    def reset_transform(self, odometry):
        t, tp = _tran(odometry); _check(self.L.cvo_reset_transform(self.h, tp))

    def reset_initial(self, odometry):
        t, tp = _tran(odometry); out = np.zeros(12, np.float32)
        _check(self.L.cvo_reset_initial(self.h, tp, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out.reshape(3, 4)

    # -- getters, cvo.hpp:268-270 + public members cvo.hpp:139-144
    def get_fixed_and_moving_number(self):
        a = C.c_int(0); b = C.c_int(0); _check(self.L.cvo_get_fixed_and_moving_number(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def get_iteration_number(self):
        a = C.c_int(0); _check(self.L.cvo_get_iteration_number(self.h, C.byref(a))); return a.value

    def get_A_nonzero(self):
        a = C.c_int(0); _check(self.L.cvo_get_A_nonzero(self.h, C.byref(a))); return a.value

    @property
    def transform(self):
        out = np.zeros(12, np.float32); _check(self.L.cvo_get_transform(self.h, out.ctypes.data_as(C.POINTER(C.c_float)))); return out.reshape(3, 4)

    @property
    def init(self):
        a = C.c_int(0); _check(self.L.cvo_get_init(self.h, C.byref(a))); return bool(a.value)

    @property
    def first_frame(self):
        a = C.c_int(0); _check(self.L.cvo_get_first_frame(self.h, C.byref(a))); return bool(a.value)

    @first_frame.setter
    def first_frame(self, v):
        _check(self.L.cvo_set_first_frame(self.h, int(bool(v))))

    def prev_accum_transform(self):
        a = np.zeros(12, np.float32); b = np.zeros(12, np.float32); fp = C.POINTER(C.c_float)
        _check(self.L.cvo_get_prev_accum_transform(self.h, a.ctypes.data_as(fp), b.ctypes.data_as(fp)))
        return a.reshape(3, 4), b.reshape(3, 4)

    def get_state(self):
        R = np.zeros(9, np.float32); T = np.zeros(3, np.float32); ell = C.c_float(0); fp = C.POINTER(C.c_float)
        _check(self.L.cvo_get_state(self.h, R.ctypes.data_as(fp), T.ctypes.data_as(fp), C.byref(ell)))
        return dict(R=R.reshape(3, 3), T=T, ell=ell.value)

    def set_state(self, R, T, ell):
        r, rp = _f(np.asarray(R).reshape(9)); t, tp = _f(np.asarray(T).reshape(3))
        _check(self.L.cvo_set_state(self.h, rp, tp, float(ell)))

    def set_workgroups(self, g: int):
        _check(self.L.cvo_set_workgroups(self.h, int(g)))

    def set_arith_mode(self, mode):
        """arithmetic mode of this handle's alignments (cvo_hip.h: cvo_set_arith_mode): CVO_ARITH_* bits, or "base" / "eigen337"."""
        _check(self.L.cvo_set_arith_mode(self.h, arith_flags(mode)))

    def arith_mode(self) -> int:
        v = C.c_int(); _check(self.L.cvo_get_arith_mode(self.h, C.byref(v))); return v.value

    def set_tail_scores(self, on):
        """cvo_set_tail_scores: the alignment queues the tracker's score block behind itself and compute_innerproduct(the result) only collects.
        False / 0 never, True / 1 every alignment, 2 (the handle's default) when the previous alignment was followed by that question"""
        _check(self.L.cvo_set_tail_scores(self.h, int(on)))

    def queued_score_count(self) -> int:
        """cvo_queued_score_count: score blocks answered by what an alignment of this object had queued behind itself"""
        n = C.c_int(0); _check(self.L.cvo_queued_score_count(self.h, C.byref(n))); return n.value

    def shared_cloud_count(self) -> int:
        """cvo_shared_cloud_count: clouds this object took from the thread's previous generation (same images) instead of generating them"""
        n = C.c_int(0); _check(self.L.cvo_shared_cloud_count(self.h, C.byref(n))); return n.value


RESULT_FLOATS = 16      # CVO_RESULT_FLOATS
COMM_ID_BYTES = 128     # CVO_COMM_ID_BYTES


def shard_range(n_pairs: int, rank: int, world: int) -> range:
    """cvo_shard_range: the contiguous block of global pair indices `rank` owns."""
    first = C.c_int(0); count = C.c_int(0)
    _check(load_library().cvo_shard_range(n_pairs, rank, world, C.byref(first), C.byref(count)))
    return range(first.value, first.value + count.value)


def shard_block(n_pairs: int, world: int) -> int:
    """cvo_shard_block: records every rank contributes to a gather (its own, then padding)."""
    return int(load_library().cvo_shard_block(n_pairs, world))


def compact_records(gathered, n_pairs: int, world: int):
    """cvo_compact_records: rank-major gathered blocks -> (n_pairs, 16) records in global pair order, first non-zero status."""
    g = np.ascontiguousarray(gathered, np.float32)
    assert g.size == world * shard_block(n_pairs, world) * RESULT_FLOATS, g.shape
    out = np.zeros((n_pairs, RESULT_FLOATS), np.float32); err = C.c_int(0); fp = C.POINTER(C.c_float)
    _check(load_library().cvo_compact_records(g.ctypes.data_as(fp), n_pairs, world, out.ctypes.data_as(fp), C.byref(err)))
    return out, err.value


def host_register(array):
    """cvo_host_register: pin + map a numpy array's memory; clouds handed over from inside it are read in place (no staging copy)."""
    a = np.asarray(array)
    assert a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
    _check(load_library().cvo_host_register(C.c_void_p(a.ctypes.data), a.nbytes))


def host_unregister(array):
    _check(load_library().cvo_host_unregister(C.c_void_p(np.asarray(array).ctypes.data)))


def comm_library_path() -> str:
    """cvo_comm_library_path: the file the RCCL bound by the C ABI was loaded from."""
    buf = C.create_string_buffer(1024)
    _check(load_library().cvo_comm_library_path(buf, 1024))
    return buf.value.decode()


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().cvo_comm_unique_id(buf))
    return buf.raw


class CvoComm:
    """One rank's RCCL communicator (one process per GPU): rank 0 makes the id, the launcher broadcasts it."""

    def __init__(self, unique_id: bytes, n_ranks: int, rank: int, device: int = 0):
        self.L = load_library(); self.h = C.c_void_p(); self.n_ranks = n_ranks; self.rank = rank
        assert len(unique_id) == COMM_ID_BYTES
        _check(self.L.cvo_comm_create(unique_id, n_ranks, rank, device, C.byref(self.h)))

    def set_gather_stream(self, on: bool):
        """cvo_comm_set_gather_stream: every gather of this communicator on one stream of its own (fallback mode, include/cvo_hip.h)."""
        _check(self.L.cvo_comm_set_gather_stream(self.h, 1 if on else 0))

    def info(self):
        """(ranks, rank) as the RCCL communicator reports them (ncclCommCount / ncclCommUserRank)."""
        n = C.c_int(0); r = C.c_int(0)
        _check(self.L.cvo_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.cvo_comm_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CvoMulti:
    """Single process, several GPUs: one batch per device, contiguous block sharding, one RCCL all-gather of the result records
    enqueued behind every device's align launch (cvo_multi_*)."""

    def __init__(self, devices, max_pairs_per_device: int, params: Params | None = None):
        self.L = load_library(); self.params = params or default_params()
        self.devices = list(devices); self.max_pairs = max_pairs_per_device
        dev = (C.c_int * len(self.devices))(*self.devices)
        self.h = C.c_void_p()
        _check(self.L.cvo_multi_create(C.byref(self.params), dev, len(self.devices), max_pairs_per_device, C.byref(self.h)))

    def batch(self, i: int) -> "CvoBatch":
        h = C.c_void_p(); _check(self.L.cvo_multi_batch(self.h, i, C.byref(h)))
        return CvoBatch._borrow(h, self.max_pairs, self.params)

    def align_async(self, n: int):
        self._n = n
        _check(self.L.cvo_multi_align_async(self.h, n))

    def align_async_v(self, n_pairs):
        """n_pairs[i] pairs on device i; every device contributes max(n_pairs) records (padding behind its own)."""
        arr = (C.c_int * len(self.devices))(*[int(v) for v in n_pairs]); self._n = max(int(v) for v in n_pairs)
        _check(self.L.cvo_multi_align_async_v(self.h, arr))

    def wait(self, from_device: int = 0):
        out = np.zeros((len(self.devices) * self._n, RESULT_FLOATS), np.float32)
        _check(self.L.cvo_multi_wait(self.h, from_device, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.cvo_multi_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CvoBatch:
    """Independent frame pairs aligned in one persistent launch (the
    keyframe<->keyframe batch of keyframe_graph.cpp:622-731; BASELINE configs 3-4)."""

    def __init__(self, max_pairs: int, params: Params | None = None, device: int = 0):
        self.L = load_library()
        self.params = params or default_params()
        self.max_pairs = max_pairs
        self.h = C.c_void_p()
        self.owned = True
        _check(self.L.cvo_batch_create(C.byref(self.params), device, max_pairs, C.byref(self.h)))

    @classmethod
    def _borrow(cls, handle, max_pairs, params):
        """A batch owned by a CvoMulti: same methods, never destroyed from here."""
        b = cls.__new__(cls)
        b.L = load_library(); b.params = params; b.max_pairs = max_pairs; b.h = handle; b.owned = False
        return b

    def gather_results(self, comm: "CvoComm", n: int, recv_device_ptr: int):
        """ONE ncclAllGather of the first n result records (the align kernel wrote them), enqueued behind the last launch on its
        stream.  n must be the same on every rank; see gather_results_padded."""
        _check(self.L.cvo_batch_gather_results(self.h, comm.h, n, C.c_void_p(recv_device_ptr)))

    def gather_results_padded(self, comm: "CvoComm", n_valid: int, n_block: int, recv_device_ptr: int, launch_status: int = 0):
        """Every rank sends n_block records: its n_valid own, then padding (status CVO_ERR_PADDING); launch_status != 0: this rank's
        launch failed, all its records carry that code -- the rank still enters the collective."""
        _check(self.L.cvo_batch_gather_results_padded(self.h, comm.h, n_valid, n_block, launch_status, C.c_void_p(recv_device_ptr)))

    def padded_records(self, n_valid: int, n_block: int, launch_status: int = 0) -> int:
        """Device address of the block this rank would send (for launchers that run the collective themselves)."""
        p = C.c_void_p()
        _check(self.L.cvo_batch_padded_records(self.h, n_valid, n_block, launch_status, C.byref(p)))
        return int(p.value)

    def result_records(self) -> int:
        """Device address of the record table the align kernel writes (n x 16 floats), valid once the launch's stream has drained."""
        p = C.c_void_p()
        _check(self.L.cvo_batch_result_records(self.h, C.byref(p)))
        return int(p.value)

    def close(self):
        if getattr(self, "h", None) and self.h.value and getattr(self, "owned", True):
            self.L.cvo_batch_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pair(self, p, fixed_xyz, fixed_feat, moving_xyz, moving_feat):
        fx, fxp, ff, ffp = _cloud_args(fixed_xyz, fixed_feat)
        mx, mxp, mf, mfp = _cloud_args(moving_xyz, moving_feat)
        _check(self.L.cvo_batch_set_pair(self.h, p, fxp, ffp, fx.shape[0], mxp, mfp, mx.shape[0]))

    @staticmethod
    def prepare_pairs(pairs):
        """pairs: sequence of (fixed_xyz, fixed_feat, moving_xyz, moving_feat).  Returns the pointer tables cvo_batch_set_pairs takes
        (and keeps the arrays alive), so that a loop handing the same host buffers over every step pays for the hand-over only."""
        fp = C.POINTER(C.c_float)
        keep = [tuple(_cloud_args(fx, ff)[0::2] + _cloud_args(mx, mf)[0::2]) for fx, ff, mx, mf in pairs]
        n = len(keep)
        tab = lambda k: (fp * n)(*[q[k].ctypes.data_as(fp) for q in keep])
        return dict(n=n, keep=keep, fx=tab(0), ff=tab(1), mx=tab(2), mf=tab(3),
                    nf=(C.c_int * n)(*[q[0].shape[0] for q in keep]), nm=(C.c_int * n)(*[q[2].shape[0] for q in keep]))

    def set_pairs(self, prepared, first: int = 0):
        """cvo_batch_set_pairs: one hand-over for all pairs of `prepared` (prepare_pairs), or of a sequence of cloud tuples."""
        pr = prepared if isinstance(prepared, dict) else self.prepare_pairs(prepared)
        _check(self.L.cvo_batch_set_pairs(self.h, first, pr["n"], pr["fx"], pr["ff"], pr["nf"], pr["mx"], pr["mf"], pr["nm"]))

    def set_pairs_images(self, images, fixed_image, moving_image, camera, first: int = 0, swap_rb: bool = False, image_stream=None):
        """cvo_batch_set_pairs_images: pairs first .. first+len(fixed_image)-1 from RGB-D images.  images: list of (bgr8, depth16), all of one
        size, each generated once on the GPU; pair k takes images[fixed_image[k]] as its fixed cloud and images[moving_image[k]] as its moving
        one.  camera = (scaling_factor, fx, fy, cx, cy).  Returns the points of each image's cloud.
        Device images (objects with __cuda_array_interface__, see device_image) are read where they are: swap_rb (one flag, or one per image) for R, G, B colour bytes,
        image_stream for the stream that wrote them (None: torch's current stream is synchronised first when the images are torch tensors)."""
        fi = np.ascontiguousarray(fixed_image, np.int32).reshape(-1); mi = np.ascontiguousarray(moving_image, np.int32).reshape(-1)
        if fi.shape != mi.shape:
            raise ValueError("fixed_image and moving_image must have one entry per pair")
        if _images_on_device(images):
            dm = _device_images(images, swap_rb)
            w, h = dm[0][1], dm[0][2]
            if any((q[1], q[2]) != (w, h) for q in dm):
                raise ValueError("all images of one call must have the same size")
            n = len(dm); cam = Camera(*[float(v) for v in camera]); descs = (DeviceImage * n)(*[q[0] for q in dm])
            pts = np.zeros(n, np.int32); ip = C.POINTER(C.c_int)
            _settle_writer(images, image_stream)
            _check(self.L.cvo_batch_set_pairs_device_images(self.h, int(first), int(fi.shape[0]), n, descs, w, h, C.byref(cam), fi.ctypes.data_as(ip),
                                                            mi.ctypes.data_as(ip), pts.ctypes.data_as(ip), _stream_arg(image_stream)))
            return pts
        ims = [Cvo._images(b, d) for b, d in images]
        if not ims:
            raise ValueError("no images")
        w, h = ims[0][2], ims[0][3]
        if any((q[2], q[3]) != (w, h) for q in ims):
            raise ValueError("all images of one call must have the same size")
        n = len(ims); cam = Camera(*[float(v) for v in camera])
        bgr = (C.c_void_p * n)(*[q[0].ctypes.data for q in ims]); dep = (C.c_void_p * n)(*[q[1].ctypes.data for q in ims])
        pts = np.zeros(n, np.int32); ip = C.POINTER(C.c_int)
        _check(self.L.cvo_batch_set_pairs_images(self.h, int(first), int(fi.shape[0]), n, bgr, dep, w, h, C.byref(cam),
                                                 fi.ctypes.data_as(ip), mi.ctypes.data_as(ip), pts.ctypes.data_as(ip)))
        return pts

    def set_pairs_clouds(self, clouds, fixed_cloud, moving_cloud, first: int = 0, cloud_stream=None):
        """cvo_batch_set_pairs_device_clouds: pairs first .. first+len(fixed_cloud)-1 from clouds in device memory.  clouds: a list of DeviceCloud,
        (xyz, feat) or (xyz, feat, feat_layout) (see device_cloud), each ingested once; pair k takes clouds[fixed_cloud[k]] and
        clouds[moving_cloud[k]].  cloud_stream: the stream that wrote them (None: torch's current stream is synchronised first for torch tensors)."""
        fi = np.ascontiguousarray(fixed_cloud, np.int32).reshape(-1); mi = np.ascontiguousarray(moving_cloud, np.int32).reshape(-1)
        if fi.shape != mi.shape:
            raise ValueError("fixed_cloud and moving_cloud must have one entry per pair")
        arr, n = _device_clouds(clouds); ip = C.POINTER(C.c_int)
        _settle_cloud_writer(clouds, cloud_stream)
        _check(self.L.cvo_batch_set_pairs_device_clouds(self.h, int(first), int(fi.shape[0]), n, arr, fi.ctypes.data_as(ip), mi.ctypes.data_as(ip),
                                                        _stream_arg(cloud_stream)))

    def advance_clouds(self, slots, clouds, cloud_stream=None):
        """cvo_batch_advance_device_clouds: clouds[k] (as for set_pairs_clouds) is the next cloud of slot slots[k]: a slot's first cloud becomes its
        fixed cloud; after that the moving cloud moves to fixed and the cloud becomes the moving one."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        arr, n = _device_clouds(clouds)
        if sl.shape[0] != n:
            raise ValueError("one slot per cloud")
        _settle_cloud_writer(clouds, cloud_stream)
        _check(self.L.cvo_batch_advance_device_clouds(self.h, n, sl.ctypes.data_as(C.POINTER(C.c_int)), arr, _stream_arg(cloud_stream)))

    # -- K-stream frame-to-frame odometry (cvo_hip.h: cvo_batch_advance_images & co): slot p is one cvo::cvo odometry object
    def advance_images(self, slots, images, cameras, cam_index=None, swap_rb: bool = False, image_stream=None):
        """cvo_batch_advance_images: images[k] = (bgr8, depth16), all of one size, is the next frame of slot slots[k], generated with camera
        cameras[cam_index[k]] (cam_index None: cameras[0] for all).  cameras: a list of (scaling_factor, fx, fy, cx, cy), or one such tuple.
        A slot's first frame becomes its fixed cloud; after that the moving cloud moves to fixed and the frame becomes the moving cloud.
        Returns the points of each image's cloud.  Device images: as for set_pairs_images."""
        if _images_on_device(images):
            args, keep = _device_list_args(slots, images, cameras, cam_index, "slot", swap_rb)
            pts = np.zeros(args[0], np.int32)
            _settle_writer(images, image_stream)
            _check(self.L.cvo_batch_advance_device_images(self.h, *args, pts.ctypes.data_as(C.POINTER(C.c_int)), _stream_arg(image_stream)))
            return pts
        ims = [Cvo._images(b, d) for b, d in images]
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        if not ims or sl.shape[0] != len(ims):
            raise ValueError("one slot per image, at least one image")
        w, h = ims[0][2], ims[0][3]
        if any((q[2], q[3]) != (w, h) for q in ims):
            raise ValueError("all images of one call must have the same size")
        if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
            cameras = [cameras]
        cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
        ci = None if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
        if ci is not None and (ci.shape[0] != len(ims) or ci.min() < 0 or ci.max() >= len(cameras)):
            raise ValueError("cam_index: one index into cameras per image")
        n = len(ims); ip = C.POINTER(C.c_int)
        bgr = (C.c_void_p * n)(*[q[0].ctypes.data for q in ims]); dep = (C.c_void_p * n)(*[q[1].ctypes.data for q in ims])
        pts = np.zeros(n, np.int32)
        _check(self.L.cvo_batch_advance_images(self.h, n, sl.ctypes.data_as(ip), bgr, dep, w, h, cams, None if ci is None else ci.ctypes.data_as(ip),
                                               pts.ctypes.data_as(ip)))
        return pts

    def stage_images(self, slots, images, cameras, cam_index=None, swap_rb: bool = False, image_stream=None):
        """cvo_batch_stage_images: the arguments of advance_images, for the slots' NEXT frames.  Their clouds are generated on the stage's own
        stream while a launch runs (call it between align_pairs_async and wait); the images may be reused as soon as the call returns.  One
        stage per batch: a second call replaces the first.  Returns the number of images staged.  Device images: as for set_pairs_images; with
        an image_stream the call does not wait on the host at all."""
        if _images_on_device(images):
            args, keep = _device_list_args(slots, images, cameras, cam_index, "slot", swap_rb)
            _settle_writer(images, image_stream)
            _check(self.L.cvo_batch_stage_device_images(self.h, *args, _stream_arg(image_stream)))
            return args[0]
        args, keep = _image_list_args(slots, images, cameras, cam_index, "slot")
        _check(self.L.cvo_batch_stage_images(self.h, *args))
        return args[0]

    def advance_staged(self):
        """cvo_batch_advance_staged: advance_images of the staged list without generating anything; returns the points of each staged cloud"""
        n = self.staged_count()[0]
        pts = np.zeros(max(1, n), np.int32)
        _check(self.L.cvo_batch_advance_staged(self.h, pts.ctypes.data_as(C.POINTER(C.c_int))))
        return pts[:n]

    def staged_count(self):
        """cvo_batch_staged_count: (images in the stage now, clouds ever taken from a stage)"""
        n = C.c_int(0); taken = C.c_longlong(0)
        _check(self.L.cvo_batch_staged_count(self.h, C.byref(n), C.byref(taken)))
        return n.value, taken.value

    def reset_stream(self, p: int):
        """cvo_batch_reset_stream: slot p becomes a fresh odometry object (no clouds, R = I, T = 0, ell = params.ell)"""
        _check(self.L.cvo_batch_reset_stream(self.h, int(p)))

    def align_pairs_async(self, slots, stream: int | None = None):
        """cvo_batch_align_pairs_async: one launch over the listed slots; results come back in list order"""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        _check(self.L.cvo_batch_align_pairs_async(self.h, sl.shape[0], sl.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(stream) if stream else None))
        self._last_slots = sl.copy()
        return sl.shape[0]

    def align_pairs(self, slots):
        return self.wait(self.align_pairs_async(slots))

    def prev_accum_transform(self, p: int):
        """cvo_batch_get_prev_accum_transform of stream slot p: (prev, accum), (3, 4) each"""
        a = np.zeros(12, np.float32); b = np.zeros(12, np.float32); fp = C.POINTER(C.c_float)
        _check(self.L.cvo_batch_get_prev_accum_transform(self.h, int(p), a.ctypes.data_as(fp), b.ctypes.data_as(fp)))
        return a.reshape(3, 4), b.reshape(3, 4)

    def set_num_want(self, num_want: int):
        """pcd_generator::num_want of the later set_pairs_images / advance_images calls (3000 by default)"""
        _check(self.L.cvo_batch_set_num_want(self.h, int(num_want)))

    def get_cloud(self, p: int, slot: int):
        """pair p's cloud in slot SLOT_FIXED / SLOT_MOVING: xyz (n, 3), feat (5, n)"""
        n = C.c_int(0)
        _check(self.L.cvo_batch_get_cloud(self.h, int(p), int(slot), None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32); feat = np.zeros((5, n.value), np.float32)
        if n.value:
            _check(self.L.cvo_batch_get_cloud(self.h, int(p), int(slot), xyz.ctypes.data_as(C.POINTER(C.c_float)), feat.ctypes.data_as(C.POINTER(C.c_float)),
                                              n.value, C.byref(n)))
        return xyz, feat

    def get_selected_points(self, p: int, slot: int):
        """the pixel (x, y) of every point of pair p's cloud in `slot`, for clouds made by set_pairs_images (empty otherwise)"""
        n = C.c_int(0)
        _check(self.L.cvo_batch_get_selected_points(self.h, int(p), int(slot), None, 0, C.byref(n)))
        px = np.zeros((n.value, 2), np.uint16)
        if n.value:
            _check(self.L.cvo_batch_get_selected_points(self.h, int(p), int(slot), px.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return px

    def set_state(self, p, R, T, ell):
        r, rp = _f(np.asarray(R).reshape(9)); t, tp = _f(np.asarray(T).reshape(3))
        _check(self.L.cvo_batch_set_state(self.h, p, rp, tp, float(ell)))

    def set_workgroups(self, g: int):
        _check(self.L.cvo_batch_set_workgroups(self.h, int(g)))

    def set_max_workgroups(self, n: int):
        _check(self.L.cvo_batch_set_max_workgroups(self.h, int(n)))

    def set_adoption(self, on: bool):
        """finished workgroups help with the pairs of their launch that still run (cvo_hip.h: cvo_batch_set_adoption)"""
        _check(self.L.cvo_batch_set_adoption(self.h, int(bool(on))))

    def set_arith_mode(self, mode):
        """arithmetic mode of the launches queued from now on (cvo_hip.h: cvo_batch_set_arith_mode): CVO_ARITH_* bits, or "base" / "eigen337"."""
        _check(self.L.cvo_batch_set_arith_mode(self.h, arith_flags(mode)))

    def arith_mode(self) -> int:
        v = C.c_int(); _check(self.L.cvo_batch_get_arith_mode(self.h, C.byref(v))); return v.value

    def set_tail_scores(self, on: bool):
        """the tracker's score block answered by the align launch itself (cvo_hip.h: cvo_batch_set_tail_scores)"""
        _check(self.L.cvo_batch_set_tail_scores(self.h, int(bool(on))))

    def last_pair_seconds(self, n: int):
        out = np.zeros(n); _check(self.L.cvo_batch_last_pair_seconds(self.h, n, out.ctypes.data_as(C.POINTER(C.c_double)))); return out

    def last_pair_spans(self, n: int):
        """(start, end) of every pair of the last launch in seconds of the device's 100 MHz clock, and the iteration a helper joined at (0 = none)"""
        t0 = np.zeros(n); t1 = np.zeros(n); j = (C.c_int * n)()
        _check(self.L.cvo_batch_last_pair_spans(self.h, n, t0.ctypes.data_as(C.POINTER(C.c_double)), t1.ctypes.data_as(C.POINTER(C.c_double)), j))
        return t0, t1, np.array(list(j))

    def last_tail_seconds(self):
        out = np.zeros(4); _check(self.L.cvo_batch_last_tail_seconds(self.h, out.ctypes.data_as(C.POINTER(C.c_double)))); return out

    def last_cull_masks(self, n: int):
        m = (C.c_ulonglong * n)(); q = (C.c_ulonglong * n)(); _check(self.L.cvo_batch_last_cull_masks(self.h, n, m, q)); return [int(x) for x in m], [int(x) for x in q]

    def last_tail_answers(self, n: int):
        m = (C.c_int * n)()
        _check(self.L.cvo_batch_last_tail_answers(self.h, n, m))
        return list(m)

    def last_adoptions(self) -> int:
        n = C.c_int(0)
        _check(self.L.cvo_batch_last_adoptions(self.h, C.byref(n)))
        return int(n.value)

    def last_adoption_retractions(self) -> int:
        n = C.c_int(0)
        _check(self.L.cvo_batch_last_adoption_retractions(self.h, C.byref(n)))
        return int(n.value)

    def reset_states(self):
        _check(self.L.cvo_batch_reset_states(self.h))

    def align_async(self, n_pairs: int, stream: int | None = None):
        _check(self.L.cvo_batch_align_async(self.h, n_pairs, C.c_void_p(stream) if stream else None))
        self._last_slots = np.arange(n_pairs, dtype=np.int32)        # (position i of the launch is slot i)

    def wait(self, n: int = 0):
        if n <= 0:
            _check(self.L.cvo_batch_wait(self.h, None, 0)); return []
        res = (PairResult * n)()
        _check(self.L.cvo_batch_wait(self.h, res, n))
        return [dict(transform=np.array(r.transform[:], np.float32).reshape(3, 4), R=np.array(r.R[:], np.float32).reshape(3, 3),
                     T=np.array(r.T[:], np.float32), ell=r.ell, iter=r.iter, A_nonzero=r.A_nonzero,
                     iterations_run=r.iterations_run, status=r.status, rebuilds=r.rebuilds, dense_fallbacks=r.dense_fallbacks) for r in res]

    def done(self) -> bool:
        """cvo_batch_done: has the last launch completed?  Never blocks."""
        d = C.c_int(0)
        _check(self.L.cvo_batch_done(self.h, C.byref(d)))
        return bool(d.value)

    def align(self, n_pairs: int):
        self.align_async(n_pairs)
        return self.wait(n_pairs)

    def last_launch(self):
        ms = C.c_float(0); it = C.c_longlong(0); ca = C.c_longlong(0)
        _check(self.L.cvo_batch_last_launch(self.h, C.byref(ms), C.byref(it), C.byref(ca)))
        nz = C.c_longlong(0)
        _check(self.L.cvo_batch_last_nonzeros(self.h, C.byref(nz)))
        grid = C.c_int(0); helpers = C.c_int(0); conc = C.c_int(0)
        _check(self.L.cvo_batch_last_launch_shape(self.h, C.byref(grid), C.byref(helpers), C.byref(conc)))
        return dict(kernel_ms=ms.value, iterations_total=it.value, candidates_total=ca.value, nonzeros_total=nz.value,
                    grid=grid.value, helpers=helpers.value, concurrent=conc.value)

    def queue_class(self):
        """cvo_batch_queue_class: (class of the batch's own stream: 0 = normal priority, 1 = the second class; hardware queues per class)."""
        cls = C.c_int(0); lim = C.c_int(0)
        _check(self.L.cvo_batch_queue_class(self.h, C.byref(cls), C.byref(lim)))
        return cls.value, lim.value

    def last_phase_seconds(self):
        out = np.zeros(10); _check(self.L.cvo_batch_last_phase_seconds(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("lists", "candidates", "cand_reduce", "linesearch", "cand_exchange", "epilogue", "lists_cull", "cand_prologue", "lists_sort", "cand_rows"), out.tolist()))

    # -- keyframe_graph.cpp:704-717 for every aligned pair, one launch
    def compute_innerproduct_lc(self, prior_tran, lc_prior_tran, lc_prior_tran_2):
        """prior_tran / lc_prior_tran / lc_prior_tran_2: (n, 3, 4) Affine3f each.  Returns one dict per pair with the
        fields of `compute_innerproduct_lc` (cvo.cpp:505-561) plus `accept` (the reference's rule)."""
        pt = np.ascontiguousarray(prior_tran, np.float32).reshape(-1, 12); n = pt.shape[0]
        lp = np.ascontiguousarray(lc_prior_tran, np.float32).reshape(n, 12); l2 = np.ascontiguousarray(lc_prior_tran_2, np.float32).reshape(n, 12)
        out = (LcScores * n)()
        f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        _check(self.L.cvo_batch_compute_innerproduct_lc(self.h, n, f(pt), f(lp), f(l2), out))
        tup = lambda r: (r.value, r.num, r.num_e)
        return [dict(inn_prior=tup(o.inn_prior), inn_lc_prior=tup(o.inn_lc_prior), inn_lc_pre=tup(o.inn_pre), inn_lc_post=tup(o.inn_post),
                     inn_fixed_pcd=tup(o.inn_fixed_pcd), inn_moving_pcd=tup(o.inn_moving_pcd),
                     post_hessian=np.array(o.post_hessian[:]).reshape(6, 6), inliers_svd=o.inliers_svd, inliers_pnpransac=o.inliers_pnpransac,
                     cos_angle=o.cos_angle, accept=bool(o.accept)) for o in out]

    # -- local_tracker.cpp:240-251 for every aligned pair, one launch queued behind the align launch
    def enqueue_innerproduct(self, n: int):
        _check(self.L.cvo_batch_enqueue_innerproduct(self.h, n))

    def innerproduct_results_raw(self, n: int):
        """cvo_batch_innerproduct_results into a ctypes array of TrackScores: the C call alone, without the per-pair Python objects below."""
        out = (TrackScores * n)()
        _check(self.L.cvo_batch_innerproduct_results(self.h, n, out))
        return out

    def innerproduct_results(self, n: int):
        """One dict per pair with the fields of `compute_innerproduct` (cvo.cpp:475-503), tran = the pair's own align() result."""
        out = self.innerproduct_results_raw(n)
        tup = lambda r: (r.value, r.num, r.num_e)
        return [dict(inn_pre=tup(o.inn_pre), inn_post=tup(o.inn_post), inn_fixed_pcd=tup(o.inn_fixed_pcd), inn_moving_pcd=tup(o.inn_moving_pcd),
                     post_hessian=np.array(o.post_hessian[:]).reshape(6, 6), inliers=o.inliers, cos_angle=o.cos_angle) for o in out]

    def compute_innerproduct(self, n: int):
        self.enqueue_innerproduct(n)
        return self.innerproduct_results(n)

    # -- not in the reference: per-point support of the last launch's pairs (cvo_hip.h, "per-point support")
    def point_support(self, pairs=None, out=None, out_stream=None):
        """For positions `pairs` of the last launch (None: all of an align(n) / align_pairs(slots) launch), the moving cloud under the pair's own
        result transform and ell against its fixed cloud.  out None: one dict of numpy arrays per pair (sum_moving, count_moving, sum_fixed,
        count_fixed).  Else out is one dict per pair of device arrays under those keys (a direction may be left out) and the kernel writes them
        itself: with an out_stream (a torch.cuda.Stream or a raw hipStream_t) that stream waits for the launch and the host does not, with None
        the call waits.  Returns out."""
        pr, sizes = self._last_pair_sizes(pairs, out)
        ip = C.POINTER(C.c_int)
        if out is None:
            arrays, _, recs = _host_records(_SUPPORT, sizes)
            _check(self.L.cvo_batch_point_support(self.h, pr.shape[0], pr.ctypes.data_as(ip), recs))
            return arrays
        recs = _device_records(_SUPPORT, out, sizes)
        _settle_support_writer(out, out_stream)
        _check(self.L.cvo_batch_point_support_device(self.h, pr.shape[0], pr.ctypes.data_as(ip), recs, _stream_arg(out_stream)))
        return out

    # -- not in the reference: point matches of the last launch's pairs (cvo_hip.h, "point matches")
    def point_matches(self, pairs=None, out=None, out_stream=None):
        """For positions `pairs` of the last launch, the moving cloud under the pair's own result transform and ell against its fixed cloud: one dict
        per pair as Cvo.point_matches returns it.  out / out_stream as point_support: out is one dict per pair of device arrays under the array keys
        (a direction may be left out) and optionally `fit` (48 bytes; api.match_fit_records reads a host copy); the kernels write them themselves."""
        pr, sizes = self._last_pair_sizes(pairs, out)
        ip = C.POINTER(C.c_int)
        if out is None:
            arrays, fits, recs = _host_records(_MATCHES, sizes)
            _check(self.L.cvo_batch_point_matches(self.h, pr.shape[0], pr.ctypes.data_as(ip), recs))
            return _match_host_results(arrays, fits)
        recs = _device_records(_MATCHES, out, sizes)
        _settle_support_writer(out, out_stream)
        _check(self.L.cvo_batch_point_matches_device(self.h, pr.shape[0], pr.ctypes.data_as(ip), recs, _stream_arg(out_stream)))
        return out

    def _last_pair_sizes(self, pairs, out):
        """(positions int32[k], [(n_moving, n_fixed)] of those positions of the last launch)"""
        last = getattr(self, "_last_slots", None)
        if pairs is None:
            if last is None and out is None:
                raise ValueError("pairs: name the positions (the launch was not started through this object, its length is not known here)")
            pairs = np.arange(len(last) if last is not None else len(out))
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1)
        sizes = []
        for i in pr:
            slot = int(last[i]) if last is not None and 0 <= i < len(last) else int(i)
            nm, nf = C.c_int(0), C.c_int(0)
            if 0 <= slot < self.max_pairs:                           # (a bad index is the library's to refuse)
                _check(self.L.cvo_batch_get_cloud(self.h, slot, SLOT_MOVING, None, None, 0, C.byref(nm)))
                _check(self.L.cvo_batch_get_cloud(self.h, slot, SLOT_FIXED, None, None, 0, C.byref(nf)))
            sizes.append((nm.value, nf.value))
        return pr, sizes

    # -- not in the reference: K start transforms per pair, scored in one launch; the next alignment can start from the best (cvo_hip.h, "pose hypotheses")
    def _hyp_args(self, trans, pairs):
        pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1)
        t, k = _hyp_trans(trans, None if pr is None else pr.shape[0])
        return t, k, t.shape[0], pr, (None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_int)))

    def score_hypotheses(self, trans, pairs=None, ell=None):
        """(values float32[count, K], nums int32[count, K], best int32[count]) for slots `pairs` (None: 0 .. count-1): each slot's moving cloud under its K
        transforms trans[i] (count x K x 3 x 4, moving -> fixed) against its fixed cloud at ell (None: params.ell).  Scores only: no state changes."""
        t, k, count, pr, prp = self._hyp_args(trans, pairs)
        recs = (InnP * max(count * k, 1))(); best = np.full(count, -1, np.int32)
        _check(self.L.cvo_batch_score_hypotheses(self.h, count, prp, k, t.ctypes.data_as(C.POINTER(C.c_float)), float(self.params.ell if ell is None else ell),
                                                 recs, best.ctypes.data_as(C.POINTER(C.c_int))))
        v, n = _inn_arrays(recs, (count, k))
        return v, n, best

    def seed_hypotheses(self, trans, pairs=None, ell=None):
        """The same launches without a host wait, and each listed slot's next alignment starts from reset_initial(its best hypothesis) on the device;
        set_state, reset_states and the set_pair* calls drop the seed.  hypothesis_results(count) returns the scores and choices."""
        t, k, count, pr, prp = self._hyp_args(trans, pairs)
        _check(self.L.cvo_batch_seed_hypotheses_async(self.h, count, prp, k, t.ctypes.data_as(C.POINTER(C.c_float)), float(self.params.ell if ell is None else ell)))
        self._seed_k = k

    def hypothesis_results(self, count: int):
        """(values[count, K], nums[count, K], best[count]) of the last seed_hypotheses call; waits for that call's kernels alone"""
        k = int(getattr(self, "_seed_k", 0))
        if k < 1:
            raise CvoError(4, "hypothesis_results: no seed_hypotheses call yet")
        recs = (InnP * max(int(count) * k, 1))(); best = np.full(max(int(count), 0), -1, np.int32)
        _check(self.L.cvo_batch_hypothesis_results(self.h, int(count), recs, best.ctypes.data_as(C.POINTER(C.c_int))))
        v, n = _inn_arrays(recs, (int(count), k))
        return v, n, best

    # -- not in the reference: value, se(3) gradient and Hessian of the inner product (cvo_hip.h, "pose models")
    def pose_models(self, trans, pairs=None, ell=None):
        """(values float32[count, K], nums int32[count, K], grads float64[count, K, 6], hess float64[count, K, 6, 6]) for slots `pairs` (None: 0 .. count-1):
        each slot's moving cloud under its K transforms trans[i] (count x K x 3 x 4, moving -> fixed) against its fixed cloud at ell (None: params.ell).
        No state changes."""
        t, k, count, pr, prp = self._hyp_args(trans, pairs)
        recs = (PoseModel * max(count * k, 1))()
        _check(self.L.cvo_batch_pose_models(self.h, count, prp, k, t.ctypes.data_as(C.POINTER(C.c_float)), float(self.params.ell if ell is None else ell), recs))
        return _model_arrays(recs, (count, k))

    def result_models(self, pairs=None):
        """(values float32[count], nums int32[count], grads float64[count, 6], hess float64[count, 6, 6]) for positions `pairs` of the last launch (None: all of
        an align(n) / align_pairs(slots) launch): each pair's model at its own result transform and ell, read from its device-resident state behind the
        align launch."""
        if pairs is None:
            last = getattr(self, "_last_slots", None)
            if last is None:
                raise ValueError("pairs: name the positions (the launch was not started through this object, its length is not known here)")
            pairs = np.arange(len(last))
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1)
        recs = (PoseModel * max(pr.shape[0], 1))()
        _check(self.L.cvo_batch_result_models(self.h, pr.shape[0], pr.ctypes.data_as(C.POINTER(C.c_int)), recs))
        return _model_arrays(recs, (pr.shape[0],))

    def results_to_device(self, dst_device_ptr: int, n: int, stream: int | None = None):
        _check(self.L.cvo_batch_results_to_device(self.h, C.c_void_p(dst_device_ptr), n, C.c_void_p(stream) if stream else None))


def _image_list_args(ids, images, cameras, cam_index, what):
    """the arguments the image-list entry points share (cvo_batch_advance_images, cvo_tracks_step_async and their stage calls): (n, ids, bgr
    pointers, depth pointers, w, h, cameras, cam_index or None) plus the arrays that must stay alive during the call"""
    ims = [Cvo._images(b, d) for b, d in images]
    sl = np.ascontiguousarray(ids, np.int32).reshape(-1)
    if not ims or sl.shape[0] != len(ims):
        raise ValueError(f"one {what} per image, at least one image")
    w, h = ims[0][2], ims[0][3]
    if any((q[2], q[3]) != (w, h) for q in ims):
        raise ValueError("all images of one call must have the same size")
    if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
        cameras = [cameras]
    cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
    ci = None if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
    if ci is not None and (ci.shape[0] != len(ims) or ci.min() < 0 or ci.max() >= len(cameras)):
        raise ValueError("cam_index: one index into cameras per image")
    n = len(ims); ip = C.POINTER(C.c_int)
    bgr = (C.c_void_p * n)(*[q[0].ctypes.data for q in ims]); dep = (C.c_void_p * n)(*[q[1].ctypes.data for q in ims])
    return (n, sl.ctypes.data_as(ip), bgr, dep, w, h, cams, None if ci is None else ci.ctypes.data_as(ip)), (ims, sl, ci)


def _pair_result_dict(r):
    return dict(transform=np.array(r.transform[:], np.float32).reshape(3, 4), R=np.array(r.R[:], np.float32).reshape(3, 3),
                T=np.array(r.T[:], np.float32), ell=r.ell, iter=r.iter, A_nonzero=r.A_nonzero,
                iterations_run=r.iterations_run, status=r.status, rebuilds=r.rebuilds, dense_fallbacks=r.dense_fallbacks)


def _track_scores_dict(o):
    tup = lambda r: (r.value, r.num, r.num_e)
    return dict(inn_pre=tup(o.inn_pre), inn_post=tup(o.inn_post), inn_fixed_pcd=tup(o.inn_fixed_pcd), inn_moving_pcd=tup(o.inn_moving_pcd),
                post_hessian=np.array(o.post_hessian[:]).reshape(6, 6), inliers=o.inliers, cos_angle=o.cos_angle)


class CvoTracks:
    """K tracker streams (cvo_hip.h: cvo_tracks_*): each stream is the pair of cvo::cvo objects local_tracker owns -- cvo_odometry (object 0) and
    cvo_keyframe (object 1) -- and a step advances every listed stream by one frame: generation, one odometry launch, reset_initial on the device,
    one keyframe launch.  The accept rule stays with the caller: `commit` takes its decision for the frames just waited for."""
    ODOMETRY, KEYFRAME = 0, 1

    def __init__(self, max_streams: int, params: Params | None = None, device: int = 0):
        self.L = load_library()
        self.params = params or default_params()
        self.max_streams = max_streams
        self.h = C.c_void_p()
        self._n = 0
        _check(self.L.cvo_tracks_create(C.byref(self.params), device, max_streams, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.cvo_tracks_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_num_want(self, num_want: int):
        _check(self.L.cvo_tracks_set_num_want(self.h, int(num_want)))

    def set_arith_mode(self, mode):
        _check(self.L.cvo_tracks_set_arith_mode(self.h, arith_flags(mode)))

    def reset(self, s: int):
        """stream s = two fresh objects"""
        _check(self.L.cvo_tracks_reset(self.h, int(s)))

    def step_async(self, streams, images, cameras, cam_index=None, stream: int | None = None, swap_rb: bool = False, image_stream=None):
        """cvo_tracks_step_async: images[k] = (bgr8, depth16), all of one size, is the next frame of stream streams[k], generated with camera
        cameras[cam_index[k]] (cam_index None: cameras[0] for all; cameras: a list of (scaling_factor, fx, fy, cx, cy), or one such tuple).
        Device images (objects with __cuda_array_interface__, see device_image) go to cvo_tracks_step_device_async: swap_rb for R, G, B colour
        bytes, image_stream for the stream that wrote them (None: torch's current stream is synchronised first for torch tensors)."""
        if _images_on_device(images):
            args, keep = _device_list_args(streams, images, cameras, cam_index, "stream", swap_rb)
            _settle_writer(images, image_stream)
            _check(self.L.cvo_tracks_step_device_async(self.h, *args, C.c_void_p(stream) if stream else None, _stream_arg(image_stream)))
            self._n = args[0]
            return args[0]
        ims = [Cvo._images(b, d) for b, d in images]
        sl = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if not ims or sl.shape[0] != len(ims):
            raise ValueError("one stream per image, at least one image")
        w, h = ims[0][2], ims[0][3]
        if any((q[2], q[3]) != (w, h) for q in ims):
            raise ValueError("all images of one call must have the same size")
        if len(cameras) == 5 and not hasattr(cameras[0], "__len__"):
            cameras = [cameras]
        cams = (Camera * len(cameras))(*[Camera(*[float(v) for v in c]) for c in cameras])
        ci = None if cam_index is None else np.ascontiguousarray(cam_index, np.int32).reshape(-1)
        if ci is not None and (ci.shape[0] != len(ims) or ci.min() < 0 or ci.max() >= len(cameras)):
            raise ValueError("cam_index: one index into cameras per image")
        n = len(ims); ip = C.POINTER(C.c_int)
        bgr = (C.c_void_p * n)(*[q[0].ctypes.data for q in ims]); dep = (C.c_void_p * n)(*[q[1].ctypes.data for q in ims])
        _check(self.L.cvo_tracks_step_async(self.h, n, sl.ctypes.data_as(ip), bgr, dep, w, h, cams, None if ci is None else ci.ctypes.data_as(ip),
                                            C.c_void_p(stream) if stream else None))
        self._n = n
        return n

    def step_clouds_async(self, streams, clouds, stream: int | None = None, cloud_stream=None):
        """cvo_tracks_step_device_clouds_async: clouds[k] (a DeviceCloud, (xyz, feat) or (xyz, feat, feat_layout), see device_cloud) is the next
        frame of stream streams[k], ingested once and held by both objects.  cloud_stream: as for CvoBatch.set_pairs_clouds."""
        sl = np.ascontiguousarray(streams, np.int32).reshape(-1)
        arr, n = _device_clouds(clouds)
        if sl.shape[0] != n:
            raise ValueError("one stream per cloud")
        _settle_cloud_writer(clouds, cloud_stream)
        _check(self.L.cvo_tracks_step_device_clouds_async(self.h, n, sl.ctypes.data_as(C.POINTER(C.c_int)), arr, C.c_void_p(stream) if stream else None,
                                                          _stream_arg(cloud_stream)))
        self._n = n
        return n

    def step_clouds(self, streams, clouds, cloud_stream=None):
        self.step_clouds_async(streams, clouds, cloud_stream=cloud_stream)
        return self.wait()

    def stage_async(self, streams, images, cameras, cam_index=None, swap_rb: bool = False, image_stream=None):
        """cvo_tracks_stage_async: the arguments of step_async, for the streams' NEXT frames -- call it between step_async / step_staged_async
        of the current step and its wait.  The images may be reused as soon as the call returns.  Returns the number of images staged.  Device images: as for
        step_async; with an image_stream the call does not wait on the host, and the images are free for work queued on that stream."""
        if _images_on_device(images):
            args, keep = _device_list_args(streams, images, cameras, cam_index, "stream", swap_rb)
            _settle_writer(images, image_stream)
            _check(self.L.cvo_tracks_stage_device_async(self.h, *args, _stream_arg(image_stream)))
            return args[0]
        args, keep = _image_list_args(streams, images, cameras, cam_index, "stream")
        _check(self.L.cvo_tracks_stage_async(self.h, *args))
        return args[0]

    def step_staged_async(self, stream: int | None = None):
        """cvo_tracks_step_staged_async: step_async of the staged list, without generating anything"""
        n = self.staged_count()[0]
        _check(self.L.cvo_tracks_step_staged_async(self.h, C.c_void_p(stream) if stream else None))
        self._n = n
        return n

    def step_staged(self):
        self.step_staged_async()
        return self.wait()

    def staged_count(self):
        """cvo_tracks_staged_count: (images in the stage now, clouds ever taken from a stage)"""
        n = C.c_int(0); taken = C.c_longlong(0)
        _check(self.L.cvo_tracks_staged_count(self.h, C.byref(n), C.byref(taken)))
        return n.value, taken.value

    def done(self) -> bool:
        d = C.c_int(0)
        _check(self.L.cvo_tracks_done(self.h, C.byref(d)))
        return bool(d.value)

    def wait_raw(self):
        """cvo_tracks_wait into a ctypes array of TrackStep, one per stream of the step in list order"""
        out = (TrackStep * max(1, self._n))()
        _check(self.L.cvo_tracks_wait(self.h, out, self._n))
        return out

    def wait(self):
        """One dict per stream of the step, in list order: phase, points, odometry / keyframe (the fields of CvoBatch.wait), odometry_scores /
        keyframe_scores (the fields of compute_innerproduct), initial_guess (3, 4)."""
        n = self._n
        return [dict(phase=o.phase, points=o.points, odometry=_pair_result_dict(o.odometry), odometry_scores=_track_scores_dict(o.odometry_scores),
                     keyframe=_pair_result_dict(o.keyframe), keyframe_scores=_track_scores_dict(o.keyframe_scores),
                     initial_guess=np.array(o.initial_guess[:], np.float32).reshape(3, 4)) for o in self.wait_raw()[:n]]

    def step(self, streams, images, cameras, cam_index=None, swap_rb: bool = False, image_stream=None):
        self.step_async(streams, images, cameras, cam_index, swap_rb=swap_rb, image_stream=image_stream)
        return self.wait()

    def commit(self, streams, accept):
        """the caller's decision for the phase-2 frames just waited for: accept -> update_previous_pcd, reject -> reset_keyframe(t_odometry)"""
        sl = np.ascontiguousarray(streams, np.int32).reshape(-1); ac = np.ascontiguousarray([1 if a else 0 for a in accept], np.int32).reshape(-1)
        if sl.shape != ac.shape:
            raise ValueError("one decision per stream")
        ip = C.POINTER(C.c_int)
        _check(self.L.cvo_tracks_commit(self.h, sl.shape[0], sl.ctypes.data_as(ip), ac.ctypes.data_as(ip)))

    # -- not in the reference: per-point support of the step just waited for (cvo_hip.h, "per-point support")
    def point_support(self, obj: int, streams, out=None, out_stream=None):
        """Between wait() of a step and the next commit() or step: for the listed streams of that step whose object `obj` (ODOMETRY / KEYFRAME)
        aligned, the step's frame at that object's result transform against the object's fixed cloud.  out / out_stream as CvoBatch.point_support."""
        sl, sizes = self._stream_pair_sizes(obj, streams)
        ip = C.POINTER(C.c_int)
        if out is None:
            arrays, _, recs = _host_records(_SUPPORT, sizes)
            _check(self.L.cvo_tracks_point_support(self.h, int(obj), sl.shape[0], sl.ctypes.data_as(ip), recs))
            return arrays
        recs = _device_records(_SUPPORT, out, sizes)
        _settle_support_writer(out, out_stream)
        _check(self.L.cvo_tracks_point_support_device(self.h, int(obj), sl.shape[0], sl.ctypes.data_as(ip), recs, _stream_arg(out_stream)))
        return out

    # -- not in the reference: point matches of the step just waited for (cvo_hip.h, "point matches")
    def point_matches(self, obj: int, streams, out=None, out_stream=None):
        """Between wait() of a step and the next commit() or step, for the listed streams whose object `obj` aligned: the step's frame at that
        object's result transform against the object's fixed cloud, one dict per stream.  out / out_stream as CvoBatch.point_matches."""
        sl, sizes = self._stream_pair_sizes(obj, streams)
        ip = C.POINTER(C.c_int)
        if out is None:
            arrays, fits, recs = _host_records(_MATCHES, sizes)
            _check(self.L.cvo_tracks_point_matches(self.h, int(obj), sl.shape[0], sl.ctypes.data_as(ip), recs))
            return _match_host_results(arrays, fits)
        recs = _device_records(_MATCHES, out, sizes)
        _settle_support_writer(out, out_stream)
        _check(self.L.cvo_tracks_point_matches_device(self.h, int(obj), sl.shape[0], sl.ctypes.data_as(ip), recs, _stream_arg(out_stream)))
        return out

    def _stream_pair_sizes(self, obj, streams):
        """(streams int32[k], [(n_moving, n_fixed)] of their object `obj`)"""
        sl = np.ascontiguousarray(streams, np.int32).reshape(-1)
        sizes = []
        for s in sl:
            nm, nf = C.c_int(0), C.c_int(0)
            if 0 <= s < self.max_streams and obj in (0, 1):          # (anything else is the library's to refuse)
                _check(self.L.cvo_tracks_get_cloud(self.h, int(s), int(obj), SLOT_MOVING, None, None, 0, C.byref(nm)))
                _check(self.L.cvo_tracks_get_cloud(self.h, int(s), int(obj), SLOT_FIXED, None, None, 0, C.byref(nf)))
            sizes.append((nm.value, nf.value))
        return sl, sizes

    def get_cloud(self, s: int, obj: int, slot: int):
        """the cloud of stream s, object ODOMETRY / KEYFRAME, slot SLOT_FIXED / SLOT_MOVING / SLOT_PREVIOUS: xyz (n, 3), feat (5, n)"""
        n = C.c_int(0); fp = C.POINTER(C.c_float)
        _check(self.L.cvo_tracks_get_cloud(self.h, int(s), int(obj), int(slot), None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32); feat = np.zeros((5, n.value), np.float32)
        if n.value:
            _check(self.L.cvo_tracks_get_cloud(self.h, int(s), int(obj), int(slot), xyz.ctypes.data_as(fp), feat.ctypes.data_as(fp), n.value, C.byref(n)))
        return xyz, feat

    def get_selected_points(self, s: int, obj: int, slot: int):
        n = C.c_int(0)
        _check(self.L.cvo_tracks_get_selected_points(self.h, int(s), int(obj), int(slot), None, 0, C.byref(n)))
        px = np.zeros((n.value, 2), np.uint16)
        if n.value:
            _check(self.L.cvo_tracks_get_selected_points(self.h, int(s), int(obj), int(slot), px.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return px

    def get_state(self, s: int, obj: int):
        R = np.zeros(9, np.float32); T = np.zeros(3, np.float32); tf = np.zeros(12, np.float32); ell = C.c_float(0); fp = C.POINTER(C.c_float)
        _check(self.L.cvo_tracks_get_state(self.h, int(s), int(obj), R.ctypes.data_as(fp), T.ctypes.data_as(fp), C.byref(ell), tf.ctypes.data_as(fp)))
        return dict(R=R.reshape(3, 3), T=T, ell=ell.value, transform=tf.reshape(3, 4))
