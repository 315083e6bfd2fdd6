"""ctypes binding of libea_hip.so (include/ea_hip.h) — the Python stub a maintainer of a Python
harness would write; the tests and bench.py drive the C-ABI through it.

There is no CPU fallback: if the shared library is missing or no gfx950 device is present the
calls raise `EAError` (never a silent numpy path).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EA_HIP_LIB") or os.path.join(_HERE, "lib", "libea_hip.so")  # EA_HIP_LIB: A/B against another build

EA_F64, EA_F32 = 0, 1
EA_OK, EA_ERR_INVALID_ARG, EA_ERR_HIP, EA_ERR_NO_DEVICE, EA_ERR_STATE, EA_ERR_ALLOC = 0, -1, -2, -3, -4, -5
LOSS_TRIVIAL, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
STRATEGY_LM, STRATEGY_DOGLEG = 0, 1
WHY = ["none", "function_tolerance", "gradient_tolerance", "parameter_tolerance",
       "max_iterations", "min_radius", "initial_eval_failed", "too_many_invalid_steps",
       "eval_failed"]
MAX_TRACE = 128

EXPORTED = [
    "ea_last_error", "ea_version", "ea_device_count", "ea_default_options",
    "ea_problem_create", "ea_problem_destroy", "ea_problem_set_points", "ea_problem_set_point_order", "ea_problem_get_point_order",
    "ea_problem_set_points_device", "ea_problem_set_dt", "ea_problem_set_dt_image_device",
    "ea_problem_set_loss", "ea_problem_set_flavour", "ea_problem_num_points",
    "ea_eval", "ea_eval_points", "ea_cost", "ea_problem_pixel_cost", "ea_solve",
    "ea_release_cached_memory", "ea_host_alloc", "ea_host_free", "ea_batch_create", "ea_batch_destroy", "ea_batch_count", "ea_batch_eval", "ea_batch_solve",
    "ea_batch_eval_poses", "ea_batch_set_poses", "ea_batch_eval_resident_poses", "ea_batch_solve_starts", "ea_solve_starts",
    "ea_batch_cost_poses", "ea_batch_cost_resident_poses", "ea_batch_search_starts", "ea_search_starts",
    "ea_solve_pyramid", "ea_solve_sharded", "ea_solve_sharded_device",
    "ea_comm_get_unique_id", "ea_comm_create", "ea_comm_create_all", "ea_comm_destroy", "ea_comm_rank", "ea_comm_size",
    "ea_comm_gather_poses", "ea_solve_sharded_comm", "ea_comm_get_info", "ea_hip_runtime_copies", "ea_tracker_create", "ea_tracker_destroy", "ea_tracker_problem", "ea_tracker_push_frame",
    "ea_batch_row_offsets", "ea_problem_num_rows", "ea_eval_rows", "ea_eval_rows_device", "ea_batch_eval_rows_device", "ea_batch_eval_rows",
    "ea_batch_set_tuning", "ea_batch_get_info", "ea_selftest_wave_reduce",
    "ea_problem_set_ref_frame", "ea_problem_set_ref_frame_masked", "ea_problem_set_now_frame", "ea_problem_debug_now_frame",
    "ea_problem_set_ref_frame_canny", "ea_problem_set_now_frame_canny", "ea_problem_debug_now_frame_canny",
    "ea_problem_set_ref_frame_ros", "ea_problem_set_now_frame_ros", "ea_problem_debug_now_frame_ros",
    "ea_problem_set_ref_frame_ros_scaled", "ea_problem_set_now_frame_ros_scaled", "ea_resize_half",
    "ea_problem_get_points", "ea_problem_get_dt",
    "ea_problem_set_distortion", "ea_problem_set_second_camera", "ea_problem_add_term", "ea_problem_clear_terms",
    "ea_default_covariance_options", "ea_problem_covariance", "ea_batch_covariance", "ea_tracker_set_covariance",
    "ea_tracker_last_covariance", "ea_problem_set_normal_prior", "ea_tracker_set_motion_prior",
    "ea_problem_set_constant_parameters", "ea_problem_get_constant_parameters",
    "ea_problem_set_weights", "ea_problem_set_weights_device", "ea_problem_get_weights", "ea_problem_set_depth_weighting",
    "ea_problem_residual_quantiles", "ea_batch_residual_quantiles", "ea_problem_get_loss", "ea_problem_set_loss_auto_scale",
    "ea_problem_get_loss_auto_scale", "ea_selftest_select",
    "ea_default_frame_params", "ea_batch_set_frames", "ea_batch_set_frames_device",
    "ea_default_canny_frame_params", "ea_batch_set_frames_canny", "ea_batch_set_frames_canny_device",
    "ea_default_ros_frame_params", "ea_batch_set_frames_ros", "ea_batch_set_frames_ros_device",
    "ea_tracker_batch_create", "ea_tracker_batch_destroy", "ea_tracker_batch_count", "ea_tracker_batch_problem",
    "ea_tracker_batch_push_frames", "ea_tracker_batch_push_frames_device", "ea_tracker_batch_reset",
    "ea_tracker_batch_set_covariance", "ea_tracker_batch_last_covariance", "ea_tracker_batch_set_motion_prior",
    "ea_tracker_batch_get_info",
    "ea_batch_set_frames_ros_pyramid", "ea_batch_set_frames_ros_pyramid_device", "ea_batch_solve_pyramid", "ea_resize_half_levels",
    "ea_tracker_batch_create_pyramid", "ea_tracker_batch_level_problem", "ea_tracker_batch_last_summaries",
    "ea_problem_pose_stats", "ea_batch_pose_stats", "ea_default_keyframe_params", "ea_tracker_batch_set_keyframes",
    "ea_tracker_batch_keyframe_state",
    "ea_pose_to_matrix", "ea_matrix_to_pose", "ea_problem_reproject", "ea_batch_reproject", "ea_batch_reproject_device",
    "ea_problem_overlay", "ea_batch_overlay", "ea_batch_overlay_device",
    "ea_problem_set_now_depth", "ea_problem_set_now_depth_device", "ea_batch_set_now_depth", "ea_batch_set_now_depth_device",
    "ea_default_depth_gate_params", "ea_problem_depth_gate", "ea_batch_depth_gate", "ea_batch_depth_gate_device",
    "ea_tracker_batch_set_depth_gate", "ea_tracker_batch_last_depth_gate",
    "ea_default_point_selection", "ea_problem_select_points", "ea_batch_select_points",
    "ea_tracker_batch_set_point_selection", "ea_tracker_batch_last_point_selection",
    "ea_default_point_merge", "ea_problem_transform_points", "ea_batch_transform_points", "ea_problem_merge_points",
    "ea_batch_merge_points", "ea_tracker_batch_set_point_carry", "ea_tracker_batch_last_point_carry",
]

# measurement hooks (edge_alignment_amd/csrc/ea_hip_dev.h): bound by bench.py, the A/B scripts and the tests that pin the
# launch patterns; not part of the drop-in boundary
EXPORTED_DEV = [
    "ea_batch_bench_eval", "ea_batch_bench_steps", "ea_batch_bench_capture", "ea_batch_bench_capture_pipelined", "ea_batch_bench_steps_riding",
    "ea_batch_bench_result", "ea_batch_bench_result_riding", "ea_batch_bench_kernel", "ea_batch_bench_rows", "ea_batch_bench_fold",
    "ea_batch_bench_resident_poses", "ea_bench_graph_floor",
]


class EAError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libea_hip error %d: %s" % (code, msg))
        self.code = code


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p)
DEVICE_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)


class Camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double),
                ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_num_consecutive_invalid_steps", C.c_int),
                ("jacobi_scaling", C.c_int), ("strategy", C.c_int),
                ("minimizer_progress_to_stdout", C.c_int), ("iterations_per_sync", C.c_int),
                ("solve_timeout_ms", C.c_double)]


class PixelCost(C.Structure):
    _fields_ = [("total_cost", C.c_double), ("mean_cost", C.c_double), ("max_cost", C.c_double),
                ("max_pixel", C.c_double * 2), ("count", C.c_int64), ("outside", C.c_int64)]


class Summary(C.Structure):
    _fields_ = [("termination", C.c_int), ("why", C.c_int), ("num_iterations", C.c_int),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("num_point_evals", C.c_int64), ("total_time_ms", C.c_double),
                ("it_cost", C.c_double * MAX_TRACE), ("it_cost_change", C.c_double * MAX_TRACE),
                ("it_gradient_max_norm", C.c_double * MAX_TRACE),
                ("it_step_norm", C.c_double * MAX_TRACE),
                ("it_relative_decrease", C.c_double * MAX_TRACE),
                ("it_radius", C.c_double * MAX_TRACE), ("it_successful", C.c_int * MAX_TRACE)]


COV_SPARSE_QR, COV_DENSE_SVD = 0, 1


class CovarianceOptions(C.Structure):
    _fields_ = [("algorithm", C.c_int), ("min_reciprocal_condition_number", C.c_double), ("null_space_rank", C.c_int),
                ("apply_loss_function", C.c_int)]


class Covariance(C.Structure):
    _fields_ = [("ok", C.c_int), ("why", C.c_int), ("rank", C.c_int), ("n_invalid", C.c_int64), ("cost", C.c_double),
                ("eigenvalues", C.c_double * 6), ("tangent", C.c_double * 36), ("qq", C.c_double * 16),
                ("qt", C.c_double * 12), ("tt", C.c_double * 9)]


class FrameParams(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("z_scaling", C.c_double), ("ref_threshold", C.c_int),
                ("now_threshold", C.c_int), ("now_median", C.c_int), ("now_normalize", C.c_int)]


class CannyFrameParams(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("z_scaling", C.c_double), ("low_threshold", C.c_double),
                ("high_threshold", C.c_double), ("now_normalize", C.c_int), ("norm_lo", C.c_double), ("norm_hi", C.c_double)]


class RosFrameParams(C.Structure):
    _fields_ = [("full_height", C.c_int), ("full_width", C.c_int), ("halvings", C.c_int), ("threshold1", C.c_double),
                ("threshold2", C.c_double)]


class PoseStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_invalid", C.c_int64), ("n_visible", C.c_int64), ("n_inlier", C.c_int64),
                ("n_flow", C.c_int64), ("sum_flow", C.c_double)]


class KeyframeParams(C.Structure):
    _fields_ = [("min_visible_fraction", C.c_double), ("min_inlier_fraction", C.c_double), ("inlier_residual", C.c_double),
                ("max_mean_flow", C.c_double), ("max_frames", C.c_int), ("margin", C.c_int)]


KEY_FIRST, KEY_SOLVE_FAILED, KEY_VISIBLE, KEY_INLIERS, KEY_FLOW, KEY_AGE = 1, 2, 4, 8, 16, 32


class KeyframeState(C.Structure):
    _fields_ = [("keyframe_push", C.c_int64), ("age", C.c_int), ("replaced", C.c_int), ("stats", PoseStats)]


class OverlayStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("inside", C.c_int64), ("outside", C.c_int64)]


EA_DEPTH_U16, EA_DEPTH_F32 = 0, 1
GATE_BEHIND, GATE_OUTSIDE, GATE_UNKNOWN, GATE_CONSISTENT, GATE_OCCLUDED, GATE_FREE = range(6)


class DepthGateParams(C.Structure):
    _fields_ = [("radius", C.c_int), ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("w_occluded", C.c_double),
                ("w_free", C.c_double), ("w_unknown", C.c_double), ("apply", C.c_int)]


class DepthGateStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_behind", C.c_int64), ("n_outside", C.c_int64), ("n_unknown", C.c_int64),
                ("n_consistent", C.c_int64), ("n_occluded", C.c_int64), ("n_free", C.c_int64)]


def default_depth_gate_params(**over):
    """ea_default_depth_gate_params with the given fields replaced"""
    prm = DepthGateParams()
    load().ea_default_depth_gate_params(C.byref(prm))
    for k, v in over.items():
        if k not in dict(DepthGateParams._fields_):
            raise TypeError("unknown depth gate parameter %r" % k)
        setattr(prm, k, int(v) if k in ("radius", "apply") else float(v))
    return prm


def depth_gate_stats_to_dict(s):
    return {k: getattr(s, k) for k, _ in DepthGateStats._fields_}


CELL_FIRST, CELL_NEAREST = 0, 1


class PointSelection(C.Structure):
    _fields_ = [("cell_px", C.c_int), ("cell_rule", C.c_int), ("outside", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("stride", C.c_int64), ("target", C.c_int64)]


class PointSelectionStats(C.Structure):
    _fields_ = [("n_before", C.c_int64), ("no_pixel", C.c_int64), ("after_cells", C.c_int64), ("n_after", C.c_int64),
                ("stride_used", C.c_int64)]


def default_point_selection(**over):
    """ea_default_point_selection with the given fields of ea_point_selection replaced"""
    prm = PointSelection()
    load().ea_default_point_selection(C.byref(prm))
    for k, v in over.items():
        if k not in dict(PointSelection._fields_):
            raise TypeError("unknown point selection parameter %r" % k)
        setattr(prm, k, int(v))
    return prm


def point_selection_stats_to_dict(s):
    return {k: getattr(s, k) for k, _ in PointSelectionStats._fields_}


class PointMerge(C.Structure):
    _fields_ = [("require_pixel", C.c_int), ("margin", C.c_int), ("max_dt", C.c_double), ("cell_px", C.c_int), ("cell_rule", C.c_int),
                ("height", C.c_int), ("width", C.c_int), ("max_carried", C.c_int64), ("weight_scale", C.c_double)]


class PointMergeStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_dst", "n_src", "no_pixel", "off_edge", "occupied", "lost_cell", "capped", "carried",
                                         "n_after")]


def default_point_merge(**over):
    """ea_default_point_merge with the given fields of ea_point_merge replaced"""
    prm = PointMerge()
    load().ea_default_point_merge(C.byref(prm))
    kinds = dict(PointMerge._fields_)
    for k, v in over.items():
        if k not in kinds:
            raise TypeError("unknown point merge parameter %r" % k)
        setattr(prm, k, float(v) if kinds[k] is C.c_double else int(v))
    return prm


def point_merge_stats_to_dict(s):
    return {k: getattr(s, k) for k, _ in PointMergeStats._fields_}


def _depth_image(depth):
    """(array kept alive, kind, height, width) of a host depth image: uint16 (TUM) or float32 (metres)"""
    if depth.dtype == np.uint16:
        kind = EA_DEPTH_U16
    elif depth.dtype == np.float32:
        kind = EA_DEPTH_F32
    else:
        raise ValueError("depth must be uint16 or float32")
    if depth.ndim != 2:
        raise ValueError("depth must be (H, W)")
    depth = np.ascontiguousarray(depth)
    return depth, kind, depth.shape[0], depth.shape[1]


def _depth_tensor(depth):
    """(address, kind, height, width) of a depth image in a torch tensor on the GPU: int16 bits of uint16, or float32"""
    import torch
    if not depth.is_cuda or not depth.is_contiguous() or depth.dim() != 2:
        raise ValueError("depth must be a contiguous (H, W) tensor on the GPU")
    if depth.dtype == torch.float32:
        kind = EA_DEPTH_F32
    elif depth.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
        kind = EA_DEPTH_U16
    else:
        raise ValueError("depth must hold uint16 (as int16 or uint16) or float32")
    torch.cuda.current_stream(depth.device).synchronize()    # the image is complete before the library copies it
    return depth.data_ptr(), kind, int(depth.shape[0]), int(depth.shape[1])


def overlay_stats_to_dict(s):
    return {k: getattr(s, k) for k, _ in OverlayStats._fields_}


def pose_stats_to_dict(s):
    return {k: getattr(s, k) for k, _ in PoseStats._fields_}


_lib = None


def load():
    """dlopen libea_hip.so and declare every prototype of include/ea_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EAError(-3, "%s not built — run `python -c 'import __graft_entry__ as g; g.build()'`; "
                          "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    i64p = C.POINTER(C.c_int64)
    L.ea_last_error.restype = C.c_char_p
    L.ea_version.restype = C.c_char_p
    L.ea_device_count.argtypes = [C.POINTER(C.c_int)]
    L.ea_default_options.argtypes = [C.POINTER(Options)]
    L.ea_default_options.restype = None
    L.ea_problem_create.argtypes = [C.POINTER(vp), C.POINTER(Camera), C.c_int, C.c_int]
    L.ea_problem_destroy.argtypes = [vp]
    L.ea_problem_destroy.restype = None
    L.ea_problem_set_points.argtypes = [vp, dp, C.c_int64, C.c_int64]
    L.ea_problem_set_points_device.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.ea_problem_set_point_order.argtypes = [vp, C.c_int]
    L.ea_problem_set_weights.argtypes = [vp, dp, C.c_int64]
    L.ea_problem_set_weights_device.argtypes = [vp, vp, C.c_int64]
    L.ea_problem_get_weights.argtypes = [vp, dp, C.c_int64, i64p]
    L.ea_problem_set_depth_weighting.argtypes = [vp, C.c_double, C.c_int]
    L.ea_problem_get_point_order.argtypes = [vp, C.POINTER(C.c_int)]
    L.ea_problem_set_dt.argtypes = [vp, dp, C.c_int, C.c_int]
    L.ea_problem_set_dt_image_device.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ea_problem_set_loss.argtypes = [vp, C.c_int, C.c_double]
    L.ea_problem_set_flavour.argtypes = [vp, C.c_double, C.c_double, C.c_int]
    L.ea_problem_num_points.argtypes = [vp]
    L.ea_problem_num_points.restype = C.c_int64
    L.ea_eval.argtypes = [vp, dp, dp, dp, dp, dp, i64p]
    L.ea_eval_points.argtypes = [vp, dp, dp, dp, dp, C.c_int]
    L.ea_cost.argtypes = [vp, dp, dp, dp, i64p]
    L.ea_solve.argtypes = [vp, C.POINTER(Options), dp, dp, C.POINTER(Summary)]
    L.ea_batch_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int]
    L.ea_batch_destroy.argtypes = [vp]
    L.ea_batch_destroy.restype = None
    L.ea_batch_count.argtypes = [vp]
    L.ea_batch_eval.argtypes = [vp, dp, dp, dp, dp, dp, i64p]
    L.ea_batch_solve.argtypes = [vp, C.POINTER(Options), dp, dp, C.POINTER(Summary)]
    L.ea_batch_eval_poses.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, i64p]
    L.ea_batch_set_poses.argtypes = [vp, C.c_int, dp, dp]
    L.ea_batch_eval_resident_poses.argtypes = [vp, dp, dp, dp, i64p]
    L.ea_batch_solve_starts.argtypes = [vp, C.c_int, C.POINTER(Options), dp, dp, C.POINTER(Summary), C.POINTER(C.c_int)]
    L.ea_solve_starts.argtypes = [vp, C.c_int, C.POINTER(Options), dp, dp, C.POINTER(Summary), C.POINTER(C.c_int)]
    L.ea_batch_cost_poses.argtypes = [vp, C.c_int, dp, dp, dp, i64p]
    L.ea_batch_cost_resident_poses.argtypes = [vp, dp, i64p]
    L.ea_batch_search_starts.argtypes = [vp, C.c_int, dp, dp, C.c_int, C.POINTER(Options), dp, dp, C.POINTER(C.c_int),
                                         C.POINTER(Summary), C.POINTER(C.c_int)]
    L.ea_search_starts.argtypes = L.ea_batch_search_starts.argtypes
    L.ea_batch_bench_eval.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, dp]
    L.ea_batch_bench_steps.argtypes = [vp, C.c_int, dp]
    L.ea_batch_bench_capture.argtypes = [vp, C.c_int]
    L.ea_batch_bench_capture_pipelined.argtypes = [vp, C.c_int]
    L.ea_batch_bench_steps_riding.argtypes = [vp, C.c_int, dp]
    L.ea_batch_bench_result.argtypes = [vp, dp, dp, dp, i64p]
    L.ea_batch_bench_result_riding.argtypes = [vp, dp, dp, dp, i64p]
    L.ea_batch_bench_kernel.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp]
    L.ea_batch_bench_fold.argtypes = [vp, C.c_int, C.c_int, dp]
    L.ea_batch_bench_resident_poses.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(C.c_int)]
    L.ea_bench_graph_floor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp]
    L.ea_batch_row_offsets.argtypes = [vp, i64p]
    L.ea_problem_num_rows.argtypes = [vp, i64p]
    L.ea_eval_rows.argtypes = [vp, dp, dp, C.c_int, C.c_int, vp, vp, C.c_int64, i64p]
    L.ea_eval_rows_device.argtypes = [vp, dp, dp, C.c_int, C.c_int, vp, vp, C.c_int64, i64p]
    L.ea_batch_eval_rows_device.argtypes = [vp, dp, dp, C.c_int, C.c_int, vp, vp, C.c_int64, i64p]
    L.ea_batch_eval_rows.argtypes = [vp, dp, dp, C.c_int, C.c_int, vp, vp, C.c_int64, i64p]
    L.ea_batch_bench_rows.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, C.c_int, C.c_int, dp]
    L.ea_problem_pixel_cost.argtypes = [vp, dp, dp, C.POINTER(PixelCost)]
    L.ea_solve_sharded.argtypes = [vp, C.POINTER(Options), ALLREDUCE_FN, vp, dp, dp, C.POINTER(Summary)]
    L.ea_solve_sharded_device.argtypes = [vp, C.POINTER(Options), DEVICE_ALLREDUCE_FN, vp, vp, dp, dp, C.POINTER(Summary)]
    L.ea_solve_pyramid.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Options), dp, dp, C.POINTER(Summary)]
    L.ea_comm_get_unique_id.argtypes = [C.c_char_p]
    L.ea_comm_create.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.ea_comm_create_all.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
    L.ea_comm_destroy.argtypes = [vp]
    L.ea_comm_destroy.restype = None
    L.ea_comm_rank.argtypes = [vp]
    L.ea_comm_size.argtypes = [vp]
    L.ea_comm_gather_poses.argtypes = [vp, vp, dp, dp, C.POINTER(C.c_int), C.c_int, dp, dp, C.POINTER(C.c_int)]
    L.ea_solve_sharded_comm.argtypes = [vp, C.POINTER(Options), vp, dp, dp, C.POINTER(Summary)]
    L.ea_comm_get_info.argtypes = [vp, C.c_char_p, i64p]
    L.ea_batch_set_tuning.argtypes = [vp, C.c_char_p, C.c_int]
    L.ea_batch_get_info.argtypes = [vp, C.c_char_p, i64p]
    L.ea_selftest_wave_reduce.argtypes = [C.c_int, C.POINTER(C.c_float), dp, dp, C.POINTER(C.c_float)]
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    L.ea_tracker_create.argtypes = [C.POINTER(vp), C.POINTER(Camera), C.c_int, C.c_int, C.c_int]
    L.ea_tracker_destroy.argtypes = [vp]
    L.ea_tracker_destroy.restype = None
    L.ea_tracker_problem.argtypes = [vp]
    L.ea_tracker_problem.restype = vp
    L.ea_tracker_push_frame.argtypes = [vp, u8p, u16p, C.c_int, C.c_int, C.c_double, C.POINTER(Options), dp, dp,
                                        C.POINTER(Summary), C.POINTER(C.c_int)]
    L.ea_problem_set_ref_frame.argtypes = [vp, u8p, u16p, C.c_int, C.c_int, C.c_double, C.c_int]
    L.ea_problem_set_now_frame.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ea_problem_set_ref_frame_masked.argtypes = [vp, u8p, u8p, u16p, C.c_int, C.c_int, C.c_double, C.c_int]
    L.ea_problem_set_ref_frame_ros.argtypes = [vp, u8p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_double, C.c_double]
    L.ea_problem_set_now_frame_ros.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_double, C.c_double]
    L.ea_problem_set_ref_frame_ros_scaled.argtypes = [vp, u8p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    L.ea_problem_set_now_frame_ros_scaled.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    L.ea_resize_half.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.ea_problem_debug_now_frame_ros.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_double, C.c_double, u8p, C.POINTER(C.c_float)]
    L.ea_problem_set_ref_frame_canny.argtypes = [vp, u8p, C.POINTER(C.c_uint16), C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    L.ea_problem_set_now_frame_canny.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]
    L.ea_problem_debug_now_frame_canny.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                                   C.c_double, u8p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.ea_problem_debug_now_frame.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    L.ea_problem_get_points.argtypes = [vp, dp, C.c_int64]
    L.ea_problem_get_dt.argtypes = [vp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ea_problem_set_distortion.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
    L.ea_problem_set_second_camera.argtypes = [vp, dp, dp]
    L.ea_problem_add_term.argtypes = [vp, vp]
    L.ea_problem_clear_terms.argtypes = [vp]
    covp, covop = C.POINTER(Covariance), C.POINTER(CovarianceOptions)
    L.ea_default_covariance_options.argtypes = [covop]
    L.ea_default_covariance_options.restype = None
    L.ea_problem_covariance.argtypes = [vp, dp, dp, covop, covp]
    L.ea_batch_covariance.argtypes = [vp, dp, dp, covop, covp]
    L.ea_tracker_set_covariance.argtypes = [vp, covop]
    L.ea_tracker_last_covariance.argtypes = [vp, covp]
    L.ea_problem_set_normal_prior.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.ea_tracker_set_motion_prior.argtypes = [vp, C.c_double, C.c_double]
    L.ea_problem_set_constant_parameters.argtypes = [vp, C.POINTER(C.c_int)]
    L.ea_problem_get_constant_parameters.argtypes = [vp, C.POINTER(C.c_int)]
    L.ea_problem_residual_quantiles.argtypes = [vp, dp, dp, dp, C.c_int, dp, i64p]
    L.ea_batch_residual_quantiles.argtypes = [vp, dp, dp, dp, C.c_int, dp, i64p]
    L.ea_problem_get_loss.argtypes = [vp, C.POINTER(C.c_int), dp]
    L.ea_problem_set_loss_auto_scale.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.ea_problem_get_loss_auto_scale.argtypes = [vp, dp, dp, dp]
    L.ea_selftest_select.argtypes = [C.c_int, dp, i64p, C.c_int, dp, C.c_int, dp, i64p]
    L.ea_default_frame_params.argtypes = [C.POINTER(FrameParams), C.c_int, C.c_int]
    L.ea_default_frame_params.restype = None
    L.ea_batch_set_frames.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(FrameParams)]
    L.ea_batch_set_frames_device.argtypes = L.ea_batch_set_frames.argtypes
    L.ea_default_canny_frame_params.argtypes = [C.POINTER(CannyFrameParams), C.c_int, C.c_int]
    L.ea_default_canny_frame_params.restype = None
    L.ea_batch_set_frames_canny.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(CannyFrameParams)]
    L.ea_batch_set_frames_canny_device.argtypes = L.ea_batch_set_frames_canny.argtypes
    L.ea_default_ros_frame_params.argtypes = [C.POINTER(RosFrameParams), C.c_int, C.c_int]
    L.ea_default_ros_frame_params.restype = None
    L.ea_batch_set_frames_ros.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(RosFrameParams)]
    L.ea_batch_set_frames_ros_device.argtypes = L.ea_batch_set_frames_ros.argtypes
    L.ea_batch_set_frames_ros_pyramid.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(RosFrameParams)]
    L.ea_batch_set_frames_ros_pyramid_device.argtypes = L.ea_batch_set_frames_ros_pyramid.argtypes
    L.ea_batch_solve_pyramid.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Options), dp, dp, C.POINTER(Summary)]
    L.ea_tracker_batch_create_pyramid.argtypes = [C.POINTER(vp), C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ea_tracker_batch_level_problem.argtypes = [vp, C.c_int, C.c_int]
    L.ea_tracker_batch_level_problem.restype = vp
    L.ea_tracker_batch_last_summaries.argtypes = [vp, C.c_int, C.POINTER(Summary)]
    L.ea_resize_half_levels.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.ea_tracker_batch_create.argtypes = [C.POINTER(vp), C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ea_tracker_batch_destroy.argtypes = [vp]
    L.ea_tracker_batch_destroy.restype = None
    L.ea_tracker_batch_count.argtypes = [vp]
    L.ea_tracker_batch_problem.argtypes = [vp, C.c_int]
    L.ea_tracker_batch_problem.restype = vp
    L.ea_tracker_batch_push_frames.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_double, C.POINTER(Options),
                                               dp, dp, C.POINTER(Summary), C.POINTER(C.c_int)]
    L.ea_tracker_batch_push_frames_device.argtypes = L.ea_tracker_batch_push_frames.argtypes
    L.ea_tracker_batch_reset.argtypes = [vp, C.c_int]
    L.ea_tracker_batch_set_covariance.argtypes = [vp, covop]
    L.ea_tracker_batch_last_covariance.argtypes = [vp, C.c_int, covp]
    L.ea_tracker_batch_set_motion_prior.argtypes = [vp, C.c_double, C.c_double]
    L.ea_tracker_batch_get_info.argtypes = [vp, C.c_char_p, i64p]
    L.ea_problem_pose_stats.argtypes = [vp, dp, dp, C.c_int, C.c_double, C.POINTER(PoseStats)]
    L.ea_batch_pose_stats.argtypes = [vp, dp, dp, C.c_int, C.c_double, C.POINTER(PoseStats)]
    L.ea_default_keyframe_params.argtypes = [C.POINTER(KeyframeParams)]
    L.ea_default_keyframe_params.restype = None
    L.ea_tracker_batch_set_keyframes.argtypes = [vp, C.POINTER(KeyframeParams)]
    L.ea_tracker_batch_keyframe_state.argtypes = [vp, C.c_int, C.POINTER(KeyframeState)]
    u8p, ovp = C.POINTER(C.c_uint8), C.POINTER(OverlayStats)
    L.ea_pose_to_matrix.argtypes = [dp, dp, dp]
    L.ea_matrix_to_pose.argtypes = [dp, dp, dp]
    L.ea_problem_reproject.argtypes = [vp, dp, dp, C.c_int64]
    L.ea_batch_reproject.argtypes = [vp, dp, dp, C.c_int64]
    L.ea_batch_reproject_device.argtypes = [vp, dp, vp, C.c_int64]
    L.ea_problem_overlay.argtypes = [vp, dp, vp, C.c_int, C.c_int, u8p, vp, ovp]
    L.ea_batch_overlay.argtypes = [vp, dp, C.POINTER(vp), C.c_int, C.c_int, u8p, C.POINTER(vp), ovp]
    L.ea_batch_overlay_device.argtypes = [vp, dp, C.POINTER(vp), C.c_int, C.c_int, u8p, ovp]
    dgp, dgs = C.POINTER(DepthGateParams), C.POINTER(DepthGateStats)
    L.ea_problem_set_now_depth.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.ea_problem_set_now_depth_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.ea_batch_set_now_depth.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_double]
    L.ea_batch_set_now_depth_device.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_double]
    L.ea_default_depth_gate_params.argtypes = [dgp]
    L.ea_default_depth_gate_params.restype = None
    L.ea_problem_depth_gate.argtypes = [vp, dp, dgp, vp, C.c_int64, dgs]
    L.ea_batch_depth_gate.argtypes = [vp, dp, dgp, vp, C.c_int64, dgs]
    L.ea_batch_depth_gate_device.argtypes = [vp, dp, dgp, vp, C.c_int64, dgs]
    L.ea_tracker_batch_set_depth_gate.argtypes = [vp, dgp]
    L.ea_tracker_batch_last_depth_gate.argtypes = [vp, C.c_int, C.c_int, dgs]
    psp, pss = C.POINTER(PointSelection), C.POINTER(PointSelectionStats)
    L.ea_default_point_selection.argtypes = [psp]
    L.ea_default_point_selection.restype = None
    L.ea_problem_select_points.argtypes = [vp, psp, pss]
    L.ea_batch_select_points.argtypes = [vp, C.POINTER(C.c_int), C.c_int, psp, pss]
    L.ea_tracker_batch_set_point_selection.argtypes = [vp, psp]
    L.ea_tracker_batch_last_point_selection.argtypes = [vp, pss, C.c_int]
    pmp, pms = C.POINTER(PointMerge), C.POINTER(PointMergeStats)
    L.ea_default_point_merge.argtypes = [pmp]
    L.ea_default_point_merge.restype = None
    L.ea_problem_transform_points.argtypes = [vp, dp]
    L.ea_batch_transform_points.argtypes = [vp, C.POINTER(C.c_int), C.c_int, dp]
    L.ea_problem_merge_points.argtypes = [vp, vp, dp, pmp, pms]
    L.ea_batch_merge_points.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(vp), dp, pmp, pms]
    L.ea_tracker_batch_set_point_carry.argtypes = [vp, pmp]
    L.ea_tracker_batch_last_point_carry.argtypes = [vp, pms, C.c_int]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise EAError(rc, load().ea_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pose_to_matrix(q, t):
    """ea_pose_to_matrix: b_T_a (4, 4) of q = (w, x, y, z) as given (not normalised) and t"""
    q, t, m = _f64(q).reshape(4), _f64(t).reshape(3), np.zeros((4, 4))
    _check(load().ea_pose_to_matrix(_dp(q), _dp(t), _dp(m)))
    return m


def matrix_to_pose(b_T_a):
    """ea_matrix_to_pose: (q, t) of a 4x4 b_T_a"""
    m, q, t = _f64(b_T_a).reshape(16), np.zeros(4), np.zeros(3)
    _check(load().ea_matrix_to_pose(_dp(m), _dp(q), _dp(t)))
    return q, t


def _pose_matrix(M):
    """a pose as the library's reprojection calls take it: a 4x4 matrix, or a (q, t) tuple converted with pose_to_matrix"""
    if isinstance(M, tuple) and len(M) == 2:
        return pose_to_matrix(*M)
    return _f64(M).reshape(4, 4)


def _pose_matrices(M, n):
    """n poses: an array (n, 4, 4), or a sequence of n entries each a matrix or a (q, t) tuple"""
    if isinstance(M, np.ndarray):
        return _f64(M).reshape(n, 4, 4)
    return _f64(np.stack([_pose_matrix(m) for m in M]) if n else np.zeros((0, 4, 4))).reshape(n, 4, 4)


def _color(color):
    if color is None:
        return None
    c = np.ascontiguousarray(color, dtype=np.uint8).reshape(3)
    return c.ctypes.data_as(C.POINTER(C.c_uint8)), c


def device_count():
    n = C.c_int(0)
    rc = load().ea_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def default_options(**kw):
    o = Options()
    load().ea_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


_TRACE_FIELDS = ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius")
_TRACE_OFF = Summary.it_cost.offset // 8


def covariance_options(**kw):
    """ea_covariance_options: defaults of ceres::Covariance::Options (SPARSE_QR, 1e-14, 0, apply_loss_function) with
    keyword overrides; algorithm may be given as "sparse_qr" / "dense_svd" """
    o = CovarianceOptions()
    load().ea_default_covariance_options(C.byref(o))
    for k, v in kw.items():
        if k == "algorithm" and isinstance(v, str):
            v = {"sparse_qr": COV_SPARSE_QR, "dense_svd": COV_DENSE_SVD}[v.lower()]
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, int(v) if k != "min_reciprocal_condition_number" else float(v))
    return o


def covariance_to_dict(c):
    """ea_covariance -> dict of numpy arrays: tangent (6, 6), qq (4, 4), qt (4, 3), tt (3, 3), eigenvalues (6,)"""
    def arr(a, shape):
        return np.frombuffer(a, dtype=np.float64).reshape(shape).copy()
    return dict(ok=bool(c.ok), why=c.why, rank=c.rank, n_invalid=c.n_invalid, cost=c.cost,
                eigenvalues=arr(c.eigenvalues, (6,)), tangent=arr(c.tangent, (6, 6)), qq=arr(c.qq, (4, 4)),
                qt=arr(c.qt, (4, 3)), tt=arr(c.tt, (3, 3)))


def summary_to_dict(s):
    ni = min(s.num_iterations + 1, MAX_TRACE)
    # one zero-copy view of the struct's six double[MAX_TRACE] arrays instead of six ctypes slices
    tr = np.frombuffer(s, dtype=np.float64, count=6 * MAX_TRACE, offset=8 * _TRACE_OFF).reshape(6, MAX_TRACE)[:, :ni].copy()
    d = dict(termination=s.termination, why=WHY[s.why], num_iterations=s.num_iterations,
             num_successful_steps=s.num_successful_steps,
             num_unsuccessful_steps=s.num_unsuccessful_steps,
             initial_cost=s.initial_cost, final_cost=s.final_cost,
             num_point_evals=s.num_point_evals, total_time_ms=s.total_time_ms,
             it_successful=np.frombuffer(s, dtype=np.int32, count=ni, offset=Summary.it_successful.offset).copy())
    for k, name in enumerate(_TRACE_FIELDS):
        d[name] = tr[k]
    return d


class Problem:
    """One frame pair: the N residual blocks + interpolator + loss of the reference's set-up
    block (standalone_edge_align.cpp:256-278), resident in HBM."""

    def __init__(self, fx, fy, cx, cy, dtype=EA_F64, device=0):
        self._h = C.c_void_p()
        cam = Camera(fx, fy, cx, cy)
        _check(load().ea_problem_create(C.byref(self._h), C.byref(cam), dtype, device))
        self.dtype = dtype
        self.device = device
        self._keep = []

    def close(self):
        if self._h:
            load().ea_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_points(self, xyz):
        xyz = _f64(xyz)
        if xyz.ndim != 2 or xyz.shape[1] < 3:
            raise ValueError("xyz must be (n, >=3)")
        _check(load().ea_problem_set_points(self._h, _dp(xyz), xyz.shape[0], xyz.shape[1]))

    def set_point_order(self, tile_px):
        """storage order for the next set_points: tiles of tile_px pixels (> 0), the caller's order (0), automatic (< 0)"""
        _check(load().ea_problem_set_point_order(self._h, int(tile_px)))

    @property
    def point_order(self):
        v = C.c_int()
        _check(load().ea_problem_get_point_order(self._h, C.byref(v)))
        return v.value

    def set_points_device(self, x_ptr, y_ptr, z_ptr, n):
        _check(load().ea_problem_set_points_device(self._h, x_ptr, y_ptr, z_ptr, n))

    def set_weights(self, w):
        """per-point weights (ceres::ScaledLoss per block), one per point in the order of set_points; None clears them"""
        if w is None:
            _check(load().ea_problem_set_weights(self._h, None, 0))
            return
        w = _f64(w).reshape(-1)
        _check(load().ea_problem_set_weights(self._h, _dp(w), w.shape[0]))

    def set_weights_device(self, w_ptr, n):
        _check(load().ea_problem_set_weights_device(self._h, w_ptr, n))

    def get_weights(self):
        """the stored weights (rounded to the problem dtype) in the caller's order, or None when no weights are set"""
        w = np.zeros(self.num_points)
        cnt = C.c_int64()
        _check(load().ea_problem_get_weights(self._h, _dp(w), w.shape[0], C.byref(cnt)))
        return w if cnt.value == w.shape[0] and cnt.value > 0 else None

    def set_depth_weighting(self, z_ref, power):
        """the reference-frame producers write w = min(1, (z_ref / z)^power) behind their points; power 0 = off"""
        _check(load().ea_problem_set_depth_weighting(self._h, float(z_ref), int(power)))

    def set_dt_grid(self, grid):
        """grid: the Grid2D view (rows = u extent, cols = v extent), row-major float64."""
        grid = _f64(grid)
        _check(load().ea_problem_set_dt(self._h, _dp(grid), grid.shape[0], grid.shape[1]))

    def set_dt_image_device(self, ptr, height, width):
        _check(load().ea_problem_set_dt_image_device(self._h, ptr, height, width))

    def set_ref_frame(self, bgr, depth_u16, z_scaling=5000.0, threshold=35, mask=None):
        """get_aX (get_aX_mask with a mask) on the GPU: bgr (H,W,3) uint8 as cv::imread returns it, depth (H,W) uint16"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_u16 = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        H, W = depth_u16.shape
        assert bgr.shape == (H, W, 3)
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.uint8)
            assert mk.shape == (H, W)
            _check(load().ea_problem_set_ref_frame_masked(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          mk.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          depth_u16.ctypes.data_as(C.POINTER(C.c_uint16)), H, W, z_scaling, threshold))
            return
        _check(load().ea_problem_set_ref_frame(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               depth_u16.ctypes.data_as(C.POINTER(C.c_uint16)), H, W, z_scaling, threshold))

    def set_now_frame(self, bgr, threshold=35, median=True, normalize=True, debug=False):
        """get_distance_transform on the GPU, written straight into the problem's DT image"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        H, W = bgr.shape[:2]
        u8 = C.POINTER(C.c_uint8)
        if not debug:
            _check(load().ea_problem_set_now_frame(self._h, bgr.ctypes.data_as(u8), H, W, threshold, int(median), int(normalize)))
            return None
        lap = np.zeros((H, W), np.uint8); mask = np.zeros((H, W), np.uint8)
        cham = np.zeros((H, W), np.int32); dt = np.zeros((H, W), np.float32)
        _check(load().ea_problem_debug_now_frame(self._h, bgr.ctypes.data_as(u8), H, W, threshold, int(median), int(normalize),
                                                 lap.ctypes.data_as(u8), mask.ctypes.data_as(u8),
                                                 cham.ctypes.data_as(C.POINTER(C.c_int32)), dt.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(lap=lap, mask=mask, chamfer=cham, dt=dt)

    def set_ref_frame_canny(self, bgr, depth_u16, z_scaling=5000.0, low=30.0, high=90.0):
        """get_aX_canny on the GPU (ref: utils.cpp:371-462)"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_u16 = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        H, W = depth_u16.shape
        assert bgr.shape == (H, W, 3)
        _check(load().ea_problem_set_ref_frame_canny(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     depth_u16.ctypes.data_as(C.POINTER(C.c_uint16)), H, W, z_scaling, low, high))

    def set_now_frame_canny(self, bgr, mask=None, low=30.0, high=90.0, normalize=(0.0, 1.0), debug=False):
        """get_distance_transform2[_masked][_NoNormalize] on the GPU (ref: utils.cpp:85-199); normalize: None or (lo, hi)"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        H, W = bgr.shape[:2]
        u8 = C.POINTER(C.c_uint8)
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.uint8)
            assert mk.shape == (H, W)
        mp = mk.ctypes.data_as(u8) if mk is not None else None
        do_norm, (lo, hi) = (0, (0.0, 1.0)) if normalize is None else (1, normalize)
        if not debug:
            _check(load().ea_problem_set_now_frame_canny(self._h, bgr.ctypes.data_as(u8), mp, H, W, low, high, do_norm, lo, hi))
            return None
        edges = np.zeros((H, W), np.uint8); cham = np.zeros((H, W), np.int32); dt = np.zeros((H, W), np.float32)
        rounds = C.c_int()
        _check(load().ea_problem_debug_now_frame_canny(self._h, bgr.ctypes.data_as(u8), mp, H, W, low, high, do_norm, lo, hi,
                                                       edges.ctypes.data_as(u8), cham.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       dt.ctypes.data_as(C.POINTER(C.c_float)), C.byref(rounds)))
        return dict(edges=edges, chamfer=cham, dt=dt, hysteresis_launches=rounds.value)

    def set_ref_frame_ros(self, bgr, depth_f32, t1=150.0, t2=100.0, halvings=0):
        """SolveEA::setRefFrame on the GPU (ref: src/SolveEA.cpp:29-82); halvings > 0: the frames are full resolution and
        the node's cv::resize x0.5 (NaN -> 0 on depth first, src/ea.cpp:38, :56-62) runs on the device that many times"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_f32 = np.ascontiguousarray(depth_f32, dtype=np.float32)
        H, W = depth_f32.shape
        assert bgr.shape == (H, W, 3)
        _check(load().ea_problem_set_ref_frame_ros_scaled(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          depth_f32.ctypes.data_as(C.POINTER(C.c_float)), H, W, int(halvings), t1, t2))

    def set_now_frame_ros(self, bgr, t1=150.0, t2=100.0, debug=False, halvings=0):
        """SolveEA::setNowFrame on the GPU (ref: src/SolveEA.cpp:86-119); halvings as in set_ref_frame_ros"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        H, W = bgr.shape[:2]
        u8 = C.POINTER(C.c_uint8)
        if halvings:
            assert not debug
            _check(load().ea_problem_set_now_frame_ros_scaled(self._h, bgr.ctypes.data_as(u8), H, W, int(halvings), t1, t2))
            return None
        if not debug:
            _check(load().ea_problem_set_now_frame_ros(self._h, bgr.ctypes.data_as(u8), H, W, t1, t2))
            return None
        edges = np.zeros((H, W), np.uint8); dt = np.zeros((H, W), np.float32)
        _check(load().ea_problem_debug_now_frame_ros(self._h, bgr.ctypes.data_as(u8), H, W, t1, t2, edges.ctypes.data_as(u8),
                                                     dt.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(edges=edges, dt=dt)

    def solve_sharded(self, q, t, allreduce, **opts):
        """ea_solve_sharded: `allreduce(array_of_32_doubles)` sums its argument in place over all ranks"""
        q, t = _f64(q).copy(), _f64(t).copy()
        o = default_options(**opts)
        s = Summary()

        def _cb(buf, count, _user):
            try:
                a = np.ctypeslib.as_array(buf, shape=(count,))
                allreduce(a)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLREDUCE_FN(_cb)
        _check(load().ea_solve_sharded(self._h, C.byref(o), cb, None, _dp(q), _dp(t), C.byref(s)))
        return q, t, summary_to_dict(s)

    def solve_sharded_device(self, q, t, enqueue_allreduce, device_sums_ptr, **opts):
        """ea_solve_sharded_device: `device_sums_ptr` = address of 32 doubles of device memory the caller owns;
        `enqueue_allreduce(stream_ptr)` must enqueue, on that HIP stream, the in-place sum of those 32 doubles over all
        ranks and return without waiting (edge_alignment_amd.dist.make_device_allreduce)."""
        q = _f64(q).reshape(4).copy()
        t = _f64(t).reshape(3).copy()
        o = default_options(**opts)
        s = Summary()

        def _cb(_buf, _count, stream, _user):
            try:
                enqueue_allreduce(stream or 0)
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = DEVICE_ALLREDUCE_FN(_cb)
        _check(load().ea_solve_sharded_device(self._h, C.byref(o), cb, None, C.c_void_p(int(device_sums_ptr)), _dp(q), _dp(t),
                                              C.byref(s)))
        return q, t, summary_to_dict(s)

    def solve_sharded_rows(self, q, t, enqueue_allreduce, agree, **opts):
        """The one-launch-per-iteration form of the point-sharded solve with the exchange supplied by the caller (what
        ea_solve_sharded_comm does with RCCL; this binding exists so that the protocol can be rehearsed over gloo):
        `enqueue_allreduce(ptr, count, stream_ptr)` enqueues the in-place sum over all ranks of `count` doubles of device
        memory at `ptr`; `agree([cannot, rows]) -> [max, max]` takes two ints to their maximum over the ranks.
        Returns (q, t, summary, used): used == 0 means some rank's shard does not qualify and nothing was solved."""
        q = _f64(q).reshape(4).copy()
        t = _f64(t).reshape(3).copy()
        o = default_options(**opts)
        s = Summary()
        used = C.c_int()

        def _cb(buf, count, stream, _user):
            try:
                enqueue_allreduce(int(buf or 0), int(count), int(stream or 0))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        def _agree(vals, _user):
            try:
                out = agree([int(vals[0]), int(vals[1])])
                vals[0], vals[1] = int(out[0]), int(out[1])
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = DEVICE_ALLREDUCE_FN(_cb)
        ag = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int), C.c_void_p)(_agree)
        L = load()
        L.ea_internal_solve_sharded_rows.restype = C.c_int
        L.ea_internal_solve_sharded_rows.argtypes = [C.c_void_p, C.c_void_p, DEVICE_ALLREDUCE_FN, type(ag), C.c_void_p, C.POINTER(C.c_double),
                                                     C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int)]
        _check(L.ea_internal_solve_sharded_rows(self._h, C.cast(C.byref(o), C.c_void_p), cb, ag, None, _dp(q), _dp(t),
                                                C.cast(C.byref(s), C.c_void_p), C.byref(used)))
        return q, t, summary_to_dict(s), used.value

    def solve_sharded_comm(self, q, t, comm, **opts):
        """ea_solve_sharded_comm: the point-sharded solve with ncclAllReduce enqueued by the library itself (no callback)"""
        q = _f64(q).reshape(4).copy()
        t = _f64(t).reshape(3).copy()
        o = default_options(**opts)
        s = Summary()
        _check(load().ea_solve_sharded_comm(self._h, C.byref(o), comm._h, _dp(q), _dp(t), C.byref(s)))
        return q, t, summary_to_dict(s)

    def pixel_cost(self, q, t):
        """the reference's integer-pixel cost report (standalone_edge_align.cpp:2494-2567) at pose (q, t)"""
        q, t = _f64(q).reshape(4), _f64(t).reshape(3)
        pc = PixelCost()
        _check(load().ea_problem_pixel_cost(self._h, _dp(q), _dp(t), C.byref(pc)))
        return dict(total_cost=pc.total_cost, mean_cost=pc.mean_cost, max_cost=pc.max_cost,
                    max_pixel=(pc.max_pixel[0], pc.max_pixel[1]), count=pc.count, outside=pc.outside)

    def get_points(self):
        n = self.num_points
        xyz = np.zeros((n, 3))
        _check(load().ea_problem_get_points(self._h, _dp(xyz), n))
        return xyz

    def get_dt(self):
        h, w = C.c_int(), C.c_int()
        _check(load().ea_problem_get_dt(self._h, None, C.byref(h), C.byref(w)))
        img = np.zeros((h.value, w.value))
        _check(load().ea_problem_get_dt(self._h, _dp(img), None, None))
        return img

    def set_distortion(self, k1, k2, p1, p2, k3):
        _check(load().ea_problem_set_distortion(self._h, k1, k2, p1, p2, k3))

    def set_second_camera(self, T12, T12inv=None):
        T12 = _f64(T12).reshape(16)
        T12inv = _f64(T12inv if T12inv is not None else np.linalg.inv(T12.reshape(4, 4))).reshape(16)
        _check(load().ea_problem_set_second_camera(self._h, _dp(T12), _dp(T12inv)))

    def add_term(self, term):
        self._keep.append(term)
        _check(load().ea_problem_add_term(self._h, term.handle))

    def clear_terms(self):
        _check(load().ea_problem_clear_terms(self._h))
        self._keep = []

    def set_loss(self, kind, a=1.0):
        _check(load().ea_problem_set_loss(self._h, kind, a))

    def get_loss(self):
        """(kind, a) the problem holds now; after a solve with auto scale: the a that solve used"""
        kind, a = C.c_int(), C.c_double()
        _check(load().ea_problem_get_loss(self._h, C.byref(kind), C.byref(a)))
        return kind.value, a.value

    def set_loss_auto_scale(self, factor, prob=0.5, a_min=1e-6):
        """every solve first sets a = max(a_min, factor * Q_prob(|r|)) at its start pose (ea_problem_set_loss_auto_scale);
        factor = 0 switches it off"""
        _check(load().ea_problem_set_loss_auto_scale(self._h, factor, prob, a_min))

    def get_loss_auto_scale(self):
        f, p, a = C.c_double(), C.c_double(), C.c_double()
        _check(load().ea_problem_get_loss_auto_scale(self._h, C.byref(f), C.byref(p), C.byref(a)))
        return f.value, p.value, a.value

    def residual_quantiles(self, q, t, probs):
        """exact order statistics of |r| over the valid blocks at (q, t): (values [len(probs)], n_valid)"""
        q, t, probs = _f64(q), _f64(t), _f64(probs).reshape(-1)
        values = np.zeros(probs.size)
        m = C.c_int64()
        _check(load().ea_problem_residual_quantiles(self._h, _dp(q), _dp(t), _dp(probs), probs.size, _dp(values), C.byref(m)))
        return values, m.value

    def pose_stats(self, q, t, margin=0, inlier_residual=float("inf")):
        """ea_problem_pose_stats at (q, t): dict n, n_invalid, n_visible, n_inlier, n_flow, sum_flow"""
        q, t = _f64(q), _f64(t)
        s = PoseStats()
        _check(load().ea_problem_pose_stats(self._h, _dp(q), _dp(t), int(margin), float(inlier_residual), C.byref(s)))
        return pose_stats_to_dict(s)

    def reproject(self, M):
        """ea_problem_reproject: (u, v) [n, 2] of the problem's own points, in the caller's order, at b_T_a = M (4x4, or a
        (q, t) tuple)"""
        M = _pose_matrix(M)
        n = self.num_points
        uv = np.zeros((max(n, 1), 2))
        _check(load().ea_problem_reproject(self._h, _dp(M), _dp(uv), n))
        return uv[:n]

    def overlay(self, M, image, color=None, out=None):
        """ea_problem_overlay: (painted copy of the uint8 H x W x 3 image, stats dict); out=image paints in place"""
        M = _pose_matrix(M)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or not image.flags.c_contiguous:
            raise ValueError("image must be a contiguous uint8 array (H, W, 3)")
        if out is None:
            out = np.empty_like(image)
        elif out.dtype != np.uint8 or out.shape != image.shape or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array of the image's shape")
        col = _color(color)
        st = OverlayStats()
        _check(load().ea_problem_overlay(self._h, _dp(M), image.ctypes.data_as(C.c_void_p), image.shape[0], image.shape[1],
                                         col[0] if col else None, out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, overlay_stats_to_dict(st)

    def set_now_depth(self, depth, z_scaling=5000.0):
        """ea_problem_set_now_depth[_device]: the current frame's depth, copied and kept in its own kind -- a uint16 (metres =
        d / z_scaling) or float32 (metres) array (H, W), or a torch tensor on the GPU (int16 / uint16 bits, or float32); None
        drops it"""
        if depth is None:
            _check(load().ea_problem_set_now_depth(self._h, None, 0, 0, 0, 0.0))
        elif hasattr(depth, "data_ptr"):
            ptr, kind, h, w = _depth_tensor(depth)
            _check(load().ea_problem_set_now_depth_device(self._h, C.c_void_p(ptr), kind, h, w, float(z_scaling)))
        else:
            depth, kind, h, w = _depth_image(depth)
            _check(load().ea_problem_set_now_depth(self._h, depth.ctypes.data_as(C.c_void_p), kind, h, w, float(z_scaling)))

    def select_points(self, **params):
        """ea_problem_select_points: thins the problem's points on the device (the reference's stride, one point per cell);
        params: the fields of ea_point_selection (cell_px, cell_rule, outside, height, width, stride, target).  Returns the
        stats dict (n_before, no_pixel, after_cells, n_after, stride_used)."""
        prm = default_point_selection(**params)
        st = PointSelectionStats()
        _check(load().ea_problem_select_points(self._h, C.byref(prm), C.byref(st)))
        return point_selection_stats_to_dict(st)

    def transform_points(self, M):
        """ea_problem_transform_points: the problem's points moved in place by a_T_o = M (4x4, or a (q, t) tuple), fp64, each
        coordinate rounded once to the problem dtype; n, order and weights stay"""
        _check(load().ea_problem_transform_points(self._h, _dp(np.ascontiguousarray(_pose_matrix(M)))))

    def merge_points(self, src, M, **params):
        """ea_problem_merge_points: the points of Problem src, moved by dst_T_src = M and filtered by the fields of
        ea_point_merge (require_pixel, margin, max_dt, cell_px, cell_rule, height, width, max_carried, weight_scale), appended
        behind this problem's own.  Returns the stats dict (n_dst, n_src, no_pixel, off_edge, occupied, lost_cell, capped,
        carried, n_after)."""
        prm = default_point_merge(**params)
        st = PointMergeStats()
        _check(load().ea_problem_merge_points(self._h, src._h, _dp(np.ascontiguousarray(_pose_matrix(M))), C.byref(prm), C.byref(st)))
        return point_merge_stats_to_dict(st)

    def depth_gate(self, M, classes=True, **params):
        """ea_problem_depth_gate at b_T_a = M (4x4, or a (q, t) tuple): (class bytes [n] in the caller's order -- None with
        classes=False --, stats dict).  params: the fields of ea_depth_gate_params (radius, abs_tol, rel_tol, w_occluded,
        w_free, w_unknown, apply) over their defaults; with apply the problem's weights are replaced"""
        M = _pose_matrix(M)
        prm = default_depth_gate_params(**params)
        n = self.num_points
        cls = np.zeros(max(n, 1), np.uint8) if classes else None
        st = DepthGateStats()
        _check(load().ea_problem_depth_gate(self._h, _dp(M), C.byref(prm), cls.ctypes.data_as(C.c_void_p) if classes else None,
                                            n, C.byref(st)))
        return (cls[:n] if classes else None), depth_gate_stats_to_dict(st)

    def set_flavour(self, z_guard=0.01, z_eps=0.0, rot_transposed=False):
        _check(load().ea_problem_set_flavour(self._h, z_guard, z_eps, int(rot_transposed)))

    @property
    def num_points(self):
        return load().ea_problem_num_points(self._h)

    def eval(self, q, t):
        q, t = _f64(q), _f64(t)
        cost = C.c_double()
        JtJ, Jtr = np.zeros((6, 6)), np.zeros(6)
        bad = C.c_int64()
        _check(load().ea_eval(self._h, _dp(q), _dp(t), C.byref(cost), _dp(JtJ), _dp(Jtr),
                              C.byref(bad)))
        return dict(cost=cost.value, JtJ=JtJ, Jtr=Jtr, n_invalid=bad.value)

    def eval_points(self, q, t, corrected=True):
        q, t = _f64(q), _f64(t)
        n = self.num_points
        r, J = np.zeros(n), np.zeros((n, 6))
        _check(load().ea_eval_points(self._h, _dp(q), _dp(t), _dp(r), _dp(J), int(corrected)))
        return r, J

    def eval_rows(self, q, t, corrected=True, layout=0):
        """materialised mode: r [rows], J [rows, 6] (layout 0) or [6, rows] (layout 1) in the problem's dtype, n_invalid"""
        q, t = _f64(q), _f64(t)
        n = C.c_int64()
        _check(load().ea_problem_num_rows(self._h, C.byref(n)))
        dt = np.float32 if self.dtype == EA_F32 else np.float64
        r = np.zeros(n.value, dtype=dt)
        J = np.zeros((n.value, 6) if layout == 0 else (6, n.value), dtype=dt)
        bad = C.c_int64()
        _check(load().ea_eval_rows(self._h, _dp(q), _dp(t), int(corrected), int(layout), r.ctypes.data_as(C.c_void_p),
                                   J.ctypes.data_as(C.c_void_p), n.value, C.byref(bad)))
        return r, J, bad.value

    def cost(self, q, t):
        q, t = _f64(q), _f64(t)
        cost, bad = C.c_double(), C.c_int64()
        _check(load().ea_cost(self._h, _dp(q), _dp(t), C.byref(cost), C.byref(bad)))
        return cost.value, bad.value

    def solve(self, q, t, **opts):
        q, t = _f64(q).copy(), _f64(t).copy()
        o = default_options(**opts)
        s = Summary()
        _check(load().ea_solve(self._h, C.byref(o), _dp(q), _dp(t), C.byref(s)))
        return q, t, summary_to_dict(s)

    def solve_starts(self, q, t, **opts):
        """K solves from K starting poses in lock-step (ea_solve_starts): q (K, 4), t (K, 3) -> (q, t, K summaries, best)"""
        q, t = _f64(q).reshape(-1, 4).copy(), _f64(t).reshape(-1, 3).copy()
        K = q.shape[0]
        assert t.shape[0] == K
        o = default_options(**opts)
        s = (Summary * K)()
        best = C.c_int(-1)
        _check(load().ea_solve_starts(self._h, K, C.byref(o), _dp(q), _dp(t), s, C.byref(best)))
        return q, t, [summary_to_dict(x) for x in s], best.value

    def search_starts(self, q, t, M, **opts):
        """rank K candidate poses by cost-only evaluation, solve the M best in lock-step (ea_search_starts): q (K, 4), t (K, 3)
        -> (q (M, 4), t (M, 3), picked (M,) candidate indices by rank, M summaries, best = index into the ranks)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        K, M = q.shape[0], int(M)
        assert t.shape[0] == K
        o = default_options(**opts)
        m = max(M, 1)
        qo, to = np.zeros((m, 4)), np.zeros((m, 3))
        picked = np.full(m, -1, dtype=np.intc)
        s = (Summary * m)()
        best = C.c_int(-1)
        _check(load().ea_search_starts(self._h, K, _dp(q), _dp(t), M, C.byref(o), _dp(qo), _dp(to),
                                       picked.ctypes.data_as(C.POINTER(C.c_int)), s, C.byref(best)))
        return qo, to, picked.astype(np.int64), [summary_to_dict(x) for x in s], best.value

    def covariance(self, q, t, **opts):
        """ceres::Covariance at (q, t) (ea_problem_covariance); opts: fields of ea_covariance_options -> covariance_to_dict"""
        q, t = _f64(q), _f64(t)
        o = covariance_options(**opts)
        c = Covariance()
        _check(load().ea_problem_covariance(self._h, _dp(q), _dp(t), C.byref(o), C.byref(c)))
        return covariance_to_dict(c)

    def set_normal_prior(self, block, A, b):
        """ceres::NormalPrior(A, b) on block 0 (q, A k x 4) or 1 (t, A k x 3) (ea_problem_set_normal_prior)"""
        n = 4 if block == 0 else 3
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        b = _f64(b).ravel()
        if block in (0, 1) and (A.ndim != 2 or A.shape[1] != n or b.size != n):  # (a bad block index: the library says so)
            raise ValueError("NormalPrior on block %d: A must be k x %d and b of size %d (got A %s, b %d)" % (block, n, n, A.shape, b.size))
        _check(load().ea_problem_set_normal_prior(self._h, int(block), _dp(A), A.shape[0], _dp(b)))

    def clear_normal_prior(self, block):
        """drops the prior on block 0 (q) or 1 (t)"""
        _check(load().ea_problem_set_normal_prior(self._h, int(block), None, 0, None))

    def set_constant_parameters(self, mask):
        """holds tangent coordinates constant, mask[6] in [delta0 delta1 delta2 | tx ty tz] order, non-zero = held; None = all
        variable (ea_problem_set_constant_parameters)"""
        _check(load().ea_problem_set_constant_parameters(self._h, _constant_mask(mask)))

    def get_constant_parameters(self):
        m = (C.c_int * 6)()
        _check(load().ea_problem_get_constant_parameters(self._h, m))
        return [int(v) for v in m]


def _constant_mask(mask):
    if mask is None:
        return None
    mask = [int(bool(v)) for v in mask]
    if len(mask) != 6:
        raise ValueError("the constant-parameter mask has 6 entries [delta0 delta1 delta2 | tx ty tz] (got %d)" % len(mask))
    return (C.c_int * 6)(*mask)


class Tracker:
    """frame-to-frame driver: push_frame aligns the previous frame's edge points against the new frame"""

    def __init__(self, fx, fy, cx, cy, dtype=EA_F64, device=0, flavour=0, loss=None):
        self._h = C.c_void_p()
        cam = Camera(fx, fy, cx, cy)
        _check(load().ea_tracker_create(C.byref(self._h), C.byref(cam), dtype, device, flavour))
        if loss is not None:
            _check(load().ea_problem_set_loss(load().ea_tracker_problem(self._h), loss[0], loss[1]))

    def push_frame(self, bgr, depth_u16, z_scaling=5000.0, **opts):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_u16 = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        H, W = depth_u16.shape
        q, t = np.zeros(4), np.zeros(3)
        o = default_options(**opts)
        s = Summary()
        aligned = C.c_int()
        _check(load().ea_tracker_push_frame(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            depth_u16.ctypes.data_as(C.POINTER(C.c_uint16)), H, W, z_scaling, C.byref(o),
                                            _dp(q), _dp(t), C.byref(s), C.byref(aligned)))
        return q, t, (summary_to_dict(s) if aligned.value else None)

    def set_covariance(self, enabled=True, **opts):
        """covariance of every aligned frame at the pose push_frame returns (ea_tracker_set_covariance); False = off"""
        o = covariance_options(**opts) if enabled else None
        _check(load().ea_tracker_set_covariance(self._h, C.byref(o) if o is not None else None))

    def set_motion_prior(self, sigma_rot, sigma_trans):
        """NormalPriors centred on each solve's start pose, A = I / sigma (ea_tracker_set_motion_prior); 0 = block off"""
        _check(load().ea_tracker_set_motion_prior(self._h, float(sigma_rot), float(sigma_trans)))

    def set_depth_weighting(self, z_ref, power):
        """ea_problem_set_depth_weighting on the tracker's problem: every reference step writes w = min(1, (z_ref / z)^power)"""
        L = load()
        _check(L.ea_problem_set_depth_weighting(L.ea_tracker_problem(self._h), float(z_ref), int(power)))

    def set_constant_parameters(self, mask):
        """the mask of ea_problem_set_constant_parameters on the tracker's problem: it holds for every push"""
        L = load()
        _check(L.ea_problem_set_constant_parameters(L.ea_tracker_problem(self._h), _constant_mask(mask)))

    def set_loss_auto_scale(self, factor, prob=0.5, a_min=1e-6):
        """ea_problem_set_loss_auto_scale on the tracker's problem: every push's solve estimates its own loss scale"""
        L = load()
        _check(L.ea_problem_set_loss_auto_scale(L.ea_tracker_problem(self._h), float(factor), float(prob), float(a_min)))

    def get_loss(self):
        """(kind, a) of the tracker's problem: after a push that aligned, the scale its solve used"""
        L = load()
        kind, a = C.c_int(), C.c_double()
        _check(L.ea_problem_get_loss(L.ea_tracker_problem(self._h), C.byref(kind), C.byref(a)))
        return kind.value, a.value

    def last_covariance(self):
        """the covariance of the last push (covariance_to_dict); EAError(EA_ERR_STATE) when it did not align"""
        c = Covariance()
        _check(load().ea_tracker_last_covariance(self._h, C.byref(c)))
        return covariance_to_dict(c)

    def close(self):
        if self._h:
            load().ea_tracker_destroy(self._h)
            self._h = C.c_void_p()


class _StreamProblem(Problem):
    """a problem owned by a TrackerBatch: every setter and read-back of Problem, no destruction"""

    def __init__(self, handle, dtype, device):
        self._h = C.c_void_p(handle)
        self.dtype = dtype
        self.device = device
        self._keep = []

    def close(self):
        self._h = C.c_void_p()


class TrackerBatch:
    """Tracker for N streams pushed in lock-step (ea_tracker_batch_*): every pushed frame passes the batched producers once
    and serves both sides, the aligned streams are solved by one batch solve.  cams: N (fx, fy, cx, cy); flavour 0 Laplacian,
    1 Canny (depth uint16), 2 ROS (depth float32 in metres, the chain works at the extent >> halvings)."""

    def __init__(self, cams, dtype=EA_F64, device=0, flavour=0, halvings=0, loss=None, levels=1):
        """levels > 1 (flavour 2): coarse-to-fine tracking, cams = [[camera per stream] per level], level 0 first, each at its
        level's working extent (frame extent >> (halvings + l)); levels = 1: cams = [camera per stream]"""
        self._h = C.c_void_p()
        L = load()
        nested = len(cams) > 0 and len(cams[0]) > 0 and isinstance(cams[0][0], (list, tuple))   # (levels = 1 given per level too)
        if levels == 1 and not nested:
            cams = [tuple(float(v) for v in c) for c in cams]
            arr = (Camera * max(len(cams), 1))(*[Camera(*c) for c in cams])
            n = len(cams)
            _check(L.ea_tracker_batch_create(C.byref(self._h), arr, n, dtype, device, flavour, halvings))
        else:
            if flavour != 2:
                raise EAError(EA_ERR_INVALID_ARG, "levels belong to the ROS flavour (2) only")
            cams = [[tuple(float(v) for v in c) for c in lv] for lv in cams]
            n = len(cams[0]) if cams else 0
            if len(cams) != levels or any(len(lv) != n for lv in cams):
                raise EAError(EA_ERR_INVALID_ARG, "cams: one list of per-stream cameras per level")
            arr = (Camera * max(levels * n, 1))(*[Camera(*c) for lv in cams for c in lv])
            _check(L.ea_tracker_batch_create_pyramid(C.byref(self._h), arr, n, levels, dtype, device, halvings))
        self.flavour, self.halvings, self.device, self.levels = flavour, halvings, device, levels
        self.problems = [_StreamProblem(L.ea_tracker_batch_problem(self._h, i), dtype, device) for i in range(n)]
        self.level_problems = [self.problems] + [[_StreamProblem(L.ea_tracker_batch_level_problem(self._h, l, i), dtype, device)
                                                  for i in range(n)] for l in range(1, levels)]
        if loss is not None:
            for p in self.problems:
                p.set_loss(loss[0], loss[1])

    def __len__(self):
        return len(self.problems)

    def problem(self, i):
        """stream i's problem: set_loss, set_loss_auto_scale, set_depth_weighting, set_constant_parameters, set_flavour;
        get_points, get_weights, get_loss"""
        return self.problems[i]

    def level_problem(self, l, i):
        """stream i's problem of pyramid level l (level 0 == problem(i))"""
        return self.level_problems[l][i]

    def last_summaries(self, i):
        """the last push's summary of stream i on every level, level 0 first; None for a level that was not solved"""
        sums = (Summary * self.levels)()
        _check(load().ea_tracker_batch_last_summaries(self._h, int(i), sums))
        zero = bytes(C.sizeof(Summary))
        return [None if bytes(s) == zero else summary_to_dict(s) for s in sums]

    def push_frames(self, bgr, depth, z_scaling=5000.0, **opts):
        """One frame per stream: sequences of len(self) frames or stacked arrays of one extent -- bgr (H, W, 3) uint8, depth
        (H, W) uint16 (float32 for flavour 2).  numpy arrays take the host entry, torch tensors on the tracker's GPU the
        device entry (read in place).  Returns q (N, 4), t (N, 3), [summary or None per stream], aligned (N,) int."""
        sides = [("bgr", bgr, 3), ("depth", depth, 4 if self.flavour == 2 else 2)]
        shape, on_device, arrays, keep = Batch._frame_arrays(self, sides)
        n = len(self)
        q, t = np.zeros((n, 4)), np.zeros((n, 3))
        o = default_options(**opts)
        sums = (Summary * n)()
        aligned = np.zeros(n, dtype=np.int32)
        if on_device:
            import torch
            torch.cuda.current_stream(self.device).synchronize()  # the frames must be complete: the producers do not wait for torch's stream
        L = load()
        fn = L.ea_tracker_batch_push_frames_device if on_device else L.ea_tracker_batch_push_frames
        H, W = shape or (0, 0)
        _check(fn(self._h, arrays["bgr"], arrays["depth"], H, W, float(z_scaling), C.byref(o), _dp(q), _dp(t), sums,
                  aligned.ctypes.data_as(C.POINTER(C.c_int))))
        return q, t, [summary_to_dict(sums[i]) if aligned[i] else None for i in range(n)], aligned

    def reset(self, i=-1):
        """stream i (default: every stream) forgets its reference and its prior"""
        _check(load().ea_tracker_batch_reset(self._h, int(i)))

    def set_covariance(self, enabled=True, **opts):
        o = covariance_options(**opts) if enabled else None
        _check(load().ea_tracker_batch_set_covariance(self._h, C.byref(o) if o is not None else None))

    def last_covariance(self, i):
        """stream i's covariance of the last push (covariance_to_dict); EAError(EA_ERR_STATE) when it was not aligned"""
        c = Covariance()
        _check(load().ea_tracker_batch_last_covariance(self._h, int(i), C.byref(c)))
        return covariance_to_dict(c)

    def set_motion_prior(self, sigma_rot, sigma_trans):
        _check(load().ea_tracker_batch_set_motion_prior(self._h, float(sigma_rot), float(sigma_trans)))

    def set_keyframes(self, params="default", **fields):
        """keyframe mode (ea_tracker_batch_set_keyframes): set_keyframes(None) = back to frame-to-frame; otherwise the defaults
        (ea_default_keyframe_params) with the given fields of ea_keyframe_params replaced"""
        if params is None:
            _check(load().ea_tracker_batch_set_keyframes(self._h, None))
            return
        prm = keyframe_params(**fields)
        _check(load().ea_tracker_batch_set_keyframes(self._h, C.byref(prm)))

    def keyframe_state(self, i):
        """stream i's keyframe state: dict keyframe_push, age, replaced (reason mask of the last push), stats (dict)"""
        s = KeyframeState()
        _check(load().ea_tracker_batch_keyframe_state(self._h, int(i), C.byref(s)))
        return {"keyframe_push": s.keyframe_push, "age": s.age, "replaced": s.replaced, "stats": pose_stats_to_dict(s.stats)}

    def set_depth_gate(self, params="default", **fields):
        """the depth gate in front of every solve of a push (ea_tracker_batch_set_depth_gate): set_depth_gate(None) = off;
        otherwise ea_default_depth_gate_params with the given fields of ea_depth_gate_params replaced (radius, abs_tol, rel_tol,
        w_occluded, w_free, w_unknown, apply).  Only while no stream holds a reference."""
        if params is None:
            _check(load().ea_tracker_batch_set_depth_gate(self._h, None))
            return
        prm = default_depth_gate_params(**fields)
        _check(load().ea_tracker_batch_set_depth_gate(self._h, C.byref(prm)))

    def set_point_selection(self, params="default", **fields):
        """point selection of every new reference (ea_tracker_batch_set_point_selection): set_point_selection(None) = off;
        otherwise ea_default_point_selection with the given fields of ea_point_selection replaced (height, width stay 0)"""
        if params is None:
            _check(load().ea_tracker_batch_set_point_selection(self._h, None))
            return
        prm = default_point_selection(**fields)
        _check(load().ea_tracker_batch_set_point_selection(self._h, C.byref(prm)))

    def set_point_carry(self, params="default", **fields):
        """points carried across a keyframe replacement (ea_tracker_batch_set_point_carry): set_point_carry(None) = off;
        otherwise ea_default_point_merge with the given fields of ea_point_merge replaced (height, width stay 0)"""
        if params is None:
            _check(load().ea_tracker_batch_set_point_carry(self._h, None))
            return
        prm = default_point_merge(**fields)
        _check(load().ea_tracker_batch_set_point_carry(self._h, C.byref(prm)))

    def last_point_carry(self):
        """[stream] stats dicts of the last push's merge (zeros: the stream did not carry)"""
        n = len(self)
        st = (PointMergeStats * max(n, 1))()
        _check(load().ea_tracker_batch_last_point_carry(self._h, st, n))
        return [point_merge_stats_to_dict(st[i]) for i in range(n)]

    def last_point_selection(self):
        """[level][stream] stats dicts: the selection of the push that took each reference (zeros: none)"""
        n = len(self)
        st = (PointSelectionStats * (self.levels * n))()
        _check(load().ea_tracker_batch_last_point_selection(self._h, st, self.levels * n))
        return [[point_selection_stats_to_dict(st[l * n + i]) for i in range(n)] for l in range(self.levels)]

    def last_depth_gate(self, i, level=0):
        """the gate's counts of stream i on `level` in the last push (depth_gate_stats_to_dict); zeros when it was not gated there"""
        st = DepthGateStats()
        _check(load().ea_tracker_batch_last_depth_gate(self._h, int(level), int(i), C.byref(st)))
        return depth_gate_stats_to_dict(st)

    def info(self, key):
        v = C.c_int64()
        _check(load().ea_tracker_batch_get_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def close(self):
        if self._h:
            for lv in self.level_problems:
                for p in lv:
                    p.close()
            load().ea_tracker_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def keyframe_params(**fields):
    """ea_default_keyframe_params with the given fields replaced"""
    prm = KeyframeParams()
    load().ea_default_keyframe_params(C.byref(prm))
    for k, v in fields.items():
        if k not in dict(KeyframeParams._fields_):
            raise TypeError("unknown keyframe parameter: " + k)
        setattr(prm, k, v)
    return prm


def solve_pyramid(levels, q, t, **opts):
    """coarse-to-fine over complete per-level problems, levels[0] = finest; returns q, t, [summary per level]"""
    q, t = _f64(q).copy(), _f64(t).copy()
    o = default_options(**opts)
    hs = (C.c_void_p * len(levels))(*[p._h for p in levels])
    s = (Summary * len(levels))()
    _check(load().ea_solve_pyramid(hs, len(levels), C.byref(o), _dp(q), _dp(t), s))
    return q, t, [summary_to_dict(x) for x in s]


def runtime_copies():
    """number of HIP runtimes mapped in this process (ea_hip_runtime_copies): 1 when torch was imported before this library"""
    return load().ea_hip_runtime_copies()


COMM_ID_BYTES = 128


def comm_unique_id():
    """the 128 bytes rank 0 hands to the other ranks (ncclGetUniqueId)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().ea_comm_get_unique_id(buf))
    return buf.raw


class Comm:
    """One RCCL communicator rank (ea_comm): the pose gather of the batch mode and the all-reduce of the point-sharded solve,
    issued by the library from librccl directly."""

    def __init__(self, unique_id, nranks, rank, device=0):
        self._h = C.c_void_p()
        assert len(unique_id) == COMM_ID_BYTES
        _check(load().ea_comm_create(C.byref(self._h), unique_id, int(nranks), int(rank), int(device)))
        self.nranks, self.rank = int(nranks), int(rank)

    @classmethod
    def from_process_group(cls, device=0):
        """inside an initialised torch.distributed group (any backend): rank 0's id broadcast as an object"""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls(box[0], world, rank, device)

    def close(self):
        if self._h:
            load().ea_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gather_poses(self, q, t, status=None, after=None):
        """-> (q (nranks * m, 4), t (nranks * m, 3), status (nranks * m,)) in rank order; `after`: the Batch that solved them"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        m = q.shape[0]
        st = np.ascontiguousarray(status if status is not None else np.zeros(m), dtype=np.int32)
        qa, ta, sa = np.zeros((self.nranks * m, 4)), np.zeros((self.nranks * m, 3)), np.zeros(self.nranks * m, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        _check(load().ea_comm_gather_poses(self._h, after._h if after is not None else None, _dp(q), _dp(t), st.ctypes.data_as(ip), m,
                                           _dp(qa), _dp(ta), sa.ctypes.data_as(ip)))
        return qa, ta, sa

    def info(self, key):
        v = C.c_int64()
        _check(load().ea_comm_get_info(self._h, key.encode(), C.byref(v)))
        return v.value


class _Pinned:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            load().ea_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def pinned_array(shape, dtype, device=0):
    """a numpy array in page-locked host memory (ea_host_alloc): frames handed to the producers / the tracker from such an
    array go up as direct DMA.  The memory is freed when the array (and every view of it) is gone."""
    L = load()
    L.ea_host_alloc.restype = C.c_void_p
    L.ea_host_alloc.argtypes = [C.c_size_t, C.c_int]
    L.ea_host_free.restype = None
    L.ea_host_free.argtypes = [C.c_void_p]
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = L.ea_host_alloc(max(n, 1), int(device))
    if not ptr:
        raise EAError(-1, L.ea_last_error().decode())
    owner = _Pinned(ptr)
    buf = (C.c_uint8 * max(n, 1)).from_address(ptr)
    buf._owner = owner   # keeps the block alive as long as the ctypes buffer (the array's base) lives
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def graph_floor_ms(device=0, nodes=200, grid=196, block=256):
    """ms per kernel node of a replayed hipGraph of EMPTY kernels (ea_bench_graph_floor): the launch mechanism's floor"""
    ms = C.c_double()
    _check(load().ea_bench_graph_floor(int(device), int(nodes), int(grid), int(block), C.byref(ms)))
    return ms.value


class Batch:
    """Several independent frame pairs evaluated / solved by the same launch sequence."""

    def __init__(self, problems):
        self.problems = list(problems)
        self.dtype = self.problems[0].dtype if self.problems else EA_F64
        arr = (C.c_void_p * len(self.problems))(*[p.handle for p in self.problems])
        self._h = C.c_void_p()
        _check(load().ea_batch_create(C.byref(self._h), arr, len(self.problems)))

    def close(self):
        if self._h:
            load().ea_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.problems)

    def eval(self, q, t):
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        n = len(self)
        cost, JtJ, Jtr = np.zeros(n), np.zeros((n, 6, 6)), np.zeros((n, 6))
        bad = np.zeros(n, dtype=np.int64)
        _check(load().ea_batch_eval(self._h, _dp(q), _dp(t), _dp(cost), _dp(JtJ), _dp(Jtr),
                                    bad.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(cost=cost, JtJ=JtJ, Jtr=Jtr, n_invalid=bad)

    def set_frames(self, ref_bgr=None, ref_depth=None, now_bgr=None, z_scaling=5000.0, ref_threshold=35, now_threshold=35,
                   median=True, normalize=True):
        """ea_batch_set_frames[_device]: Problem.set_ref_frame + Problem.set_now_frame for every problem of the batch in one
        launch sequence, bit for bit.  Each argument: a sequence of len(self) frames or one stacked array -- bgr (H, W, 3)
        uint8, depth (H, W) uint16 -- of equal extent.  numpy arrays take the host entry; torch tensors on the batch's GPU
        (contiguous; depth as torch.uint16 or int16 bits) take the device entry and are read in place.  ref_bgr and
        ref_depth go together; a side left None is not set."""
        sides = [("ref_bgr", ref_bgr, 3), ("ref_depth", ref_depth, 2), ("now_bgr", now_bgr, 3)]
        if (ref_bgr is None) != (ref_depth is None) or all(v is None for _, v, _ in sides):
            raise ValueError("ref_bgr and ref_depth go together, and one side must be given")
        shape, on_device, arrays, keep = self._frame_arrays(sides)
        L = load()
        prm = FrameParams()
        L.ea_default_frame_params(C.byref(prm), *(shape or (0, 0)))
        prm.z_scaling, prm.ref_threshold, prm.now_threshold = float(z_scaling), int(ref_threshold), int(now_threshold)
        prm.now_median, prm.now_normalize = int(bool(median)), int(bool(normalize))
        if on_device:
            import torch
            torch.cuda.current_stream(self.problems[0].device).synchronize()  # the frames must be complete: the producers do not wait for torch's stream
        fn = L.ea_batch_set_frames_device if on_device else L.ea_batch_set_frames
        _check(fn(self._h, arrays["ref_bgr"], arrays["ref_depth"], arrays["now_bgr"], C.byref(prm)))

    def _frame_arrays(self, sides):
        """the arguments of a batched producer call, sides = [(name, frames or None, kind)] with kind 3: bgr (H, W, 3) uint8,
        2: depth (H, W) uint16, 4: depth (H, W) float32, 1: mask (H, W) uint8 -> (the frames' extent, whether they are device tensors, {name: array of
        len(self) pointers or None}, what keeps the host frames alive)"""
        n = len(self)
        frames = {}
        for name, v, _ in sides:
            if v is None:
                continue
            fr = list(v) if isinstance(v, (list, tuple)) else [v[i] for i in range(len(v))]
            if len(fr) != n:
                raise EAError(EA_ERR_INVALID_ARG, "%s: %d frames for a batch of %d problems" % (name, len(fr), n))
            frames[name] = fr
        present = [f for fr in frames.values() for f in fr if f is not None]
        on_device = {type(f).__module__.split(".")[0] == "torch" for f in present}
        if len(on_device) > 1:
            raise ValueError("a mix of host arrays and device tensors")
        on_device = bool(present) and on_device.pop()
        device = self.problems[0].device
        shape, keep, arrays = None, [], {}
        for name, v, ch in sides:
            if name not in frames:
                arrays[name] = None
                continue
            ptrs = (C.c_void_p * n)()
            for i, f in enumerate(frames[name]):
                if f is None:
                    continue  # (a NULL entry: the library refuses the call)
                if on_device:
                    import torch
                    want = ((torch.float32,) if ch == 4 else (torch.uint8,) if ch != 2 else
                            (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ()))
                    if not f.is_cuda or f.device.index != device:
                        raise ValueError("%s[%d]: not a tensor on the batch's GPU %d" % (name, i, device))
                    if f.dtype not in want or not f.is_contiguous():
                        raise ValueError("%s[%d]: a contiguous %s tensor is expected" % (name, i, want[-1]))
                    ptrs[i] = f.data_ptr()
                else:
                    f = np.ascontiguousarray(f, dtype=np.float32 if ch == 4 else np.uint8 if ch != 2 else np.uint16)
                    keep.append(f)
                    ptrs[i] = f.ctypes.data
                hw = tuple(f.shape[:2])
                if tuple(f.shape) != (hw + (3,) if ch == 3 else hw) or (shape is not None and hw != shape):
                    raise ValueError("%s[%d]: shape %s; every frame of a call has one extent" % (name, i, tuple(f.shape)))
                shape = hw
            arrays[name] = ptrs
        return shape, on_device, arrays, keep

    def set_frames_canny(self, ref_bgr=None, ref_depth=None, now_bgr=None, now_mask=None, z_scaling=5000.0, low=30.0, high=90.0,
                         normalize=(0.0, 1.0)):
        """ea_batch_set_frames_canny[_device]: Problem.set_ref_frame_canny + Problem.set_now_frame_canny for every problem of
        the batch in one launch sequence, bit for bit.  The frames as for set_frames; now_mask: (H, W) uint8 per current
        frame, edges survive where mask > 1.  normalize: (lo, hi), or None for no normalisation."""
        sides = [("ref_bgr", ref_bgr, 3), ("ref_depth", ref_depth, 2), ("now_bgr", now_bgr, 3), ("now_mask", now_mask, 1)]
        if (ref_bgr is None) != (ref_depth is None) or all(v is None for _, v, _ in sides[:3]):
            raise ValueError("ref_bgr and ref_depth go together, and one side must be given")
        shape, on_device, arrays, keep = self._frame_arrays(sides)
        L = load()
        prm = CannyFrameParams()
        L.ea_default_canny_frame_params(C.byref(prm), *(shape or (0, 0)))
        prm.z_scaling, prm.low_threshold, prm.high_threshold = float(z_scaling), float(low), float(high)
        prm.now_normalize = int(normalize is not None)
        if normalize is not None:
            prm.norm_lo, prm.norm_hi = float(normalize[0]), float(normalize[1])
        if on_device:
            import torch
            torch.cuda.current_stream(self.problems[0].device).synchronize()  # (as in set_frames)
        fn = L.ea_batch_set_frames_canny_device if on_device else L.ea_batch_set_frames_canny
        _check(fn(self._h, arrays["ref_bgr"], arrays["ref_depth"], arrays["now_bgr"], arrays["now_mask"], C.byref(prm)))

    def set_frames_ros(self, ref_bgr=None, ref_depth=None, now_bgr=None, t1=150.0, t2=100.0, halvings=0):
        """ea_batch_set_frames_ros[_device]: Problem.set_ref_frame_ros + Problem.set_now_frame_ros (with their halvings) for
        every problem of the batch in one launch sequence, bit for bit.  The frames as for set_frames, at FULL resolution;
        ref_depth: (H, W) float32 in metres (numpy, or torch.float32 tensors on the batch's GPU).  A current frame without
        any edge raises EAError(EA_ERR_STATE) after everything else has been set: info("frames_without_edges")."""
        sides = [("ref_bgr", ref_bgr, 3), ("ref_depth", ref_depth, 4), ("now_bgr", now_bgr, 3)]
        if (ref_bgr is None) != (ref_depth is None) or all(v is None for _, v, _ in sides):
            raise ValueError("ref_bgr and ref_depth go together, and one side must be given")
        shape, on_device, arrays, keep = self._frame_arrays(sides)
        L = load()
        prm = RosFrameParams()
        L.ea_default_ros_frame_params(C.byref(prm), *(shape or (0, 0)))
        prm.halvings, prm.threshold1, prm.threshold2 = int(halvings), float(t1), float(t2)
        if on_device:
            import torch
            torch.cuda.current_stream(self.problems[0].device).synchronize()  # (as in set_frames)
        fn = L.ea_batch_set_frames_ros_device if on_device else L.ea_batch_set_frames_ros
        _check(fn(self._h, arrays["ref_bgr"], arrays["ref_depth"], arrays["now_bgr"], C.byref(prm)))

    def residual_quantiles(self, q, t, probs):
        """ea_batch_residual_quantiles at q (n, 4), t (n, 3): (values [n, len(probs)], n_valid [n]), one launch sequence"""
        q, t, probs = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3), _f64(probs).reshape(-1)
        n = len(self)
        values, m = np.zeros((n, probs.size)), np.zeros(n, dtype=np.int64)
        _check(load().ea_batch_residual_quantiles(self._h, _dp(q), _dp(t), _dp(probs), probs.size, _dp(values),
                                                  m.ctypes.data_as(C.POINTER(C.c_int64))))
        return values, m

    def pose_stats(self, q, t, margin=0, inlier_residual=float("inf")):
        """ea_batch_pose_stats at q (n, 4), t (n, 3): one dict per problem (Problem.pose_stats' bits), two launches"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        out = (PoseStats * max(len(self), 1))()
        _check(load().ea_batch_pose_stats(self._h, _dp(q), _dp(t), int(margin), float(inlier_residual), out))
        return [pose_stats_to_dict(out[i]) for i in range(len(self))]

    def reproject(self, M, out=None):
        """ea_batch_reproject at the poses M (n matrices, or (q, t) tuples): (u, v) [rows, 2] in the layout of row_offsets(),
        the head families' rows in storage order (rows of terms are left as they are in `out`, zero in a fresh array)"""
        M = _pose_matrices(M, len(self))
        uv = np.zeros((int(self.row_offsets()[-1]), 2)) if out is None else out
        if uv.dtype != np.float64 or not uv.flags.c_contiguous or uv.ndim != 2 or uv.shape[1] != 2:
            raise ValueError("out must be a contiguous float64 array (rows, 2)")
        _check(load().ea_batch_reproject(self._h, _dp(M), _dp(uv), uv.shape[0]))
        return uv

    def reproject_device(self, M, uv, capacity_rows=None):
        """ea_batch_reproject_device into a float64 torch tensor (rows, 2) on the batch's GPU, or a raw device address (then
        capacity_rows is required)"""
        M = _pose_matrices(M, len(self))
        if hasattr(uv, "data_ptr"):
            import torch
            if not uv.is_cuda or uv.dtype != torch.float64 or not uv.is_contiguous():
                raise ValueError("uv must be a contiguous float64 tensor on the batch's GPU")
            rows = uv.numel() // 2
            capacity_rows = rows if capacity_rows is None else min(int(capacity_rows), rows)
            torch.cuda.current_stream(uv.device).synchronize()   # the tensor's producers are done before the library writes
            uv = uv.data_ptr()
        if capacity_rows is None:
            raise ValueError("capacity_rows is required with a raw address")
        _check(load().ea_batch_reproject_device(self._h, _dp(M), C.c_void_p(uv), int(capacity_rows)))

    def overlay(self, M, images, color=None, in_place=False):
        """ea_batch_overlay: images = n uint8 (H, W, 3) arrays of one extent; returns (painted copies -- the arrays
        themselves with in_place --, list of stats dicts)"""
        M = _pose_matrices(M, len(self))
        n = len(self)
        if len(images) != n:
            raise ValueError("one image per problem")
        for im in images:
            if im.dtype != np.uint8 or im.shape != images[0].shape or im.ndim != 3 or im.shape[2] != 3 or not im.flags.c_contiguous:
                raise ValueError("images must be contiguous uint8 arrays (H, W, 3) of one extent")
        outs = list(images) if in_place else [np.empty_like(im) for im in images]
        src = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in images])
        dst = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in outs])
        col = _color(color)
        st = (OverlayStats * max(n, 1))()
        h, w = (images[0].shape[0], images[0].shape[1]) if n else (1, 1)
        _check(load().ea_batch_overlay(self._h, _dp(M), src, h, w, col[0] if col else None, dst, st))
        return outs, [overlay_stats_to_dict(st[i]) for i in range(n)]

    def overlay_device(self, M, images, color=None, height=None, width=None):
        """ea_batch_overlay_device: images = n uint8 torch tensors (H, W, 3) on the batch's GPU (or raw device addresses with
        height, width), painted in place; returns the list of stats dicts"""
        M = _pose_matrices(M, len(self))
        n = len(self)
        if len(images) != n:
            raise ValueError("one image per problem")
        ptrs = []
        for im in images:
            if hasattr(im, "data_ptr"):
                import torch
                if not im.is_cuda or im.dtype != torch.uint8 or not im.is_contiguous() or im.dim() != 3 or im.shape[2] != 3:
                    raise ValueError("images must be contiguous uint8 tensors (H, W, 3) on the batch's GPU")
                if height is None:
                    height, width = int(im.shape[0]), int(im.shape[1])
                if (int(im.shape[0]), int(im.shape[1])) != (height, width):
                    raise ValueError("images must share one extent")
                torch.cuda.current_stream(im.device).synchronize()   # the images are complete before the library paints
                ptrs.append(im.data_ptr())
            else:
                ptrs.append(int(im))
        if height is None or width is None:
            raise ValueError("height and width are required with raw addresses")
        arr = (C.c_void_p * max(n, 1))(*ptrs)
        col = _color(color)
        st = (OverlayStats * max(n, 1))()
        _check(load().ea_batch_overlay_device(self._h, _dp(M), arr, int(height), int(width), col[0] if col else None, st))
        return [overlay_stats_to_dict(st[i]) for i in range(n)]

    def set_now_depth(self, depths, z_scaling=5000.0):
        """ea_batch_set_now_depth[_device]: one depth image per problem, all uint16 or all float32 arrays (H, W) of one extent,
        or all torch tensors on the GPU; None drops every problem's image"""
        n = len(self)
        if depths is None:
            _check(load().ea_batch_set_now_depth(self._h, None, 0, 0, 0, 0.0))
            return
        if len(depths) != n:
            raise ValueError("one depth image per problem")
        on_device = n > 0 and hasattr(depths[0], "data_ptr")
        items = [_depth_tensor(d) if on_device else _depth_image(d) for d in depths]
        if len({it[1:] for it in items}) > 1:
            raise ValueError("the depth images must share one kind and extent")
        _, kind, h, w = items[0] if n else (None, 0, 3, 3)
        arr = (C.c_void_p * max(n, 1))(*[it[0] if on_device else it[0].ctypes.data for it in items])
        fn = load().ea_batch_set_now_depth_device if on_device else load().ea_batch_set_now_depth
        _check(fn(self._h, arr, kind, h, w, float(z_scaling)))

    def select_points(self, sel=None, **params):
        """ea_batch_select_points over the problems sel (batch indices, each at most once; None: every problem): one launch
        sequence and one wait.  params: the fields of ea_point_selection.  Returns the stats dicts in the order of sel."""
        prm = default_point_selection(**params)
        n = len(self) if sel is None else len(sel)
        arr = None if sel is None else (C.c_int * max(n, 1))(*[int(i) for i in sel])
        st = (PointSelectionStats * max(n, 1))()
        _check(load().ea_batch_select_points(self._h, arr, n, C.byref(prm), st))
        return [point_selection_stats_to_dict(st[i]) for i in range(n)]

    def transform_points(self, M, sel=None):
        """ea_batch_transform_points: the points of the problems sel (batch indices, each at most once; None: every problem)
        moved in place, problem sel[j] by M[j]: one launch and one wait"""
        n = len(self) if sel is None else len(sel)
        M = np.ascontiguousarray(_pose_matrices(M, n))
        arr = None if sel is None else (C.c_int * max(n, 1))(*[int(i) for i in sel])
        _check(load().ea_batch_transform_points(self._h, arr, n, _dp(M)))

    def merge_points(self, src, M, sel=None, **params):
        """ea_batch_merge_points: problem sel[j] of the batch (None: every problem) takes the points of Problem src[j] moved by
        dst_T_src = M[j]: one launch sequence and one wait.  params: the fields of ea_point_merge.  Returns the stats dicts in
        the order of sel."""
        prm = default_point_merge(**params)
        n = len(self) if sel is None else len(sel)
        if len(src) != n:
            raise ValueError("one src problem per dst problem")
        M = np.ascontiguousarray(_pose_matrices(M, n))
        arr = None if sel is None else (C.c_int * max(n, 1))(*[int(i) for i in sel])
        srcs = (C.c_void_p * max(n, 1))(*[s._h for s in src])
        st = (PointMergeStats * max(n, 1))()
        _check(load().ea_batch_merge_points(self._h, arr, n, srcs, _dp(M), C.byref(prm), st))
        return [point_merge_stats_to_dict(st[i]) for i in range(n)]

    def depth_gate(self, M, out=None, classes=True, **params):
        """ea_batch_depth_gate at the poses M: (class bytes [rows] in the layout of row_offsets(), the head families' rows in
        storage order, rows of terms as they are in `out` (zero in a fresh array) -- None with classes=False --, list of
        stats dicts)"""
        M = _pose_matrices(M, len(self))
        prm = default_depth_gate_params(**params)
        n = len(self)
        cls = None
        if classes:
            cls = np.zeros(int(self.row_offsets()[-1]), np.uint8) if out is None else out
            if cls.dtype != np.uint8 or not cls.flags.c_contiguous or cls.ndim != 1:
                raise ValueError("out must be a contiguous uint8 array (rows,)")
        st = (DepthGateStats * max(n, 1))()
        _check(load().ea_batch_depth_gate(self._h, _dp(M), C.byref(prm), cls.ctypes.data_as(C.c_void_p) if classes else None,
                                          cls.shape[0] if classes else 0, st))
        return cls, [depth_gate_stats_to_dict(st[i]) for i in range(n)]

    def depth_gate_device(self, M, cls=None, capacity_rows=None, **params):
        """ea_batch_depth_gate_device: the class bytes into a uint8 torch tensor (rows,) on the batch's GPU (or a raw device
        address with capacity_rows), or nowhere (cls=None); nothing but the stats crosses the bus.  Returns the stats dicts"""
        M = _pose_matrices(M, len(self))
        prm = default_depth_gate_params(**params)
        n = len(self)
        if cls is not None and hasattr(cls, "data_ptr"):
            import torch
            if not cls.is_cuda or cls.dtype != torch.uint8 or not cls.is_contiguous():
                raise ValueError("cls must be a contiguous uint8 tensor on the batch's GPU")
            rows = cls.numel()
            capacity_rows = rows if capacity_rows is None else min(int(capacity_rows), rows)
            torch.cuda.current_stream(cls.device).synchronize()   # the tensor's producers are done before the library writes
            cls = cls.data_ptr()
        if cls is not None and capacity_rows is None:
            raise ValueError("capacity_rows is required with a raw address")
        st = (DepthGateStats * max(n, 1))()
        _check(load().ea_batch_depth_gate_device(self._h, _dp(M), C.byref(prm), C.c_void_p(cls) if cls is not None else None,
                                                 int(capacity_rows or 0), st))
        return [depth_gate_stats_to_dict(st[i]) for i in range(n)]

    def covariance(self, q, t, **opts):
        """ea_batch_covariance: one covariance per problem at q (n, 4), t (n, 3) -> list of covariance_to_dict"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        o = covariance_options(**opts)
        out = (Covariance * len(self))()
        _check(load().ea_batch_covariance(self._h, _dp(q), _dp(t), C.byref(o), out))
        return [covariance_to_dict(c) for c in out]

    def _pose_outputs(self, K):
        n = len(self)
        return (np.zeros((K, n)), np.zeros((K, n, 6, 6)), np.zeros((K, n, 6)), np.zeros((K, n), dtype=np.int64))

    def eval_poses(self, q, t):
        """K evaluations of every problem at K different poses in one call (ea_batch_eval_poses): q (K, n, 4), t (K, n, 3)
        -> dict of cost (K, n), JtJ (K, n, 6, 6), Jtr (K, n, 6), n_invalid (K, n)"""
        n = len(self)
        q, t = _f64(q).reshape(-1, n, 4), _f64(t).reshape(-1, n, 3)
        K = q.shape[0]
        assert t.shape[0] == K
        cost, JtJ, Jtr, bad = self._pose_outputs(K)
        _check(load().ea_batch_eval_poses(self._h, K, _dp(q), _dp(t), _dp(cost), _dp(JtJ), _dp(Jtr),
                                          bad.ctypes.data_as(C.POINTER(C.c_int64))))
        self._resident_K = K
        return dict(cost=cost, JtJ=JtJ, Jtr=Jtr, n_invalid=bad)

    def set_poses(self, q, t):
        """make K poses per problem resident in HBM (ea_batch_set_poses); returns K"""
        n = len(self)
        q, t = _f64(q).reshape(-1, n, 4), _f64(t).reshape(-1, n, 3)
        assert q.shape[0] == t.shape[0]
        _check(load().ea_batch_set_poses(self._h, q.shape[0], _dp(q), _dp(t)))
        self._resident_K = q.shape[0]
        return q.shape[0]

    def eval_resident_poses(self, out=None, fetch=True):
        """the K evaluations of the resident poses (ea_batch_eval_resident_poses); `out`: arrays of a previous call to fill
        again (no allocation inside a timed region); fetch=False: run and synchronise, hand nothing back"""
        if not fetch:
            _check(load().ea_batch_eval_resident_poses(self._h, None, None, None, None))
            return None
        if out is None:
            cost, JtJ, Jtr, bad = self._pose_outputs(self._resident_K)
            out = dict(cost=cost, JtJ=JtJ, Jtr=Jtr, n_invalid=bad)
        ptrs = out.get("_ptrs")
        if ptrs is None:   # (the ctypes pointer objects of the four arrays, built once: ~2 us each -- as much as two 5e4-point evaluations)
            ptrs = out["_ptrs"] = (_dp(out["cost"]), _dp(out["JtJ"]), _dp(out["Jtr"]), out["n_invalid"].ctypes.data_as(C.POINTER(C.c_int64)))
        _check(load().ea_batch_eval_resident_poses(self._h, *ptrs))
        return out

    def cost_poses(self, q, t):
        """cost-only evaluation of every problem at K poses (ea_batch_cost_poses): q (K, n, 4), t (K, n, 3) -> dict of
        cost (K, n), n_invalid (K, n); the poses stay resident"""
        n = len(self)
        q, t = _f64(q).reshape(-1, n, 4), _f64(t).reshape(-1, n, 3)
        K = q.shape[0]
        assert t.shape[0] == K
        cost, bad = np.zeros((K, n)), np.zeros((K, n), dtype=np.int64)
        _check(load().ea_batch_cost_poses(self._h, K, _dp(q), _dp(t), _dp(cost), bad.ctypes.data_as(C.POINTER(C.c_int64))))
        self._resident_K = K
        return dict(cost=cost, n_invalid=bad)

    def cost_resident_poses(self, out=None, fetch=True):
        """the cost-only evaluation of the resident poses (ea_batch_cost_resident_poses); `out`: the dict of a previous call to
        fill again; fetch=False: run and synchronise, hand nothing back"""
        if not fetch:
            _check(load().ea_batch_cost_resident_poses(self._h, None, None))
            return None
        if out is None:
            K, n = self._resident_K, len(self)
            out = dict(cost=np.zeros((K, n)), n_invalid=np.zeros((K, n), dtype=np.int64))
        ptrs = out.get("_ptrs")
        if ptrs is None:
            ptrs = out["_ptrs"] = (_dp(out["cost"]), out["n_invalid"].ctypes.data_as(C.POINTER(C.c_int64)))
        _check(load().ea_batch_cost_resident_poses(self._h, *ptrs))
        return out

    def search_starts(self, q, t, M, summaries=True, **opts):
        """rank K candidate poses per problem by cost-only evaluation and solve the M best of each in lock-step
        (ea_batch_search_starts): q (K, n, 4), t (K, n, 3) -> (q (M, n, 4), t (M, n, 3), picked (M, n) candidate indices by
        rank, M lists of n summaries (None with summaries=False), best (n,) = index into the ranks).  Afterwards the K
        candidates are the batch's resident poses."""
        n = len(self)
        q, t = _f64(q).reshape(-1, n, 4), _f64(t).reshape(-1, n, 3)
        K, M = q.shape[0], int(M)
        assert t.shape[0] == K
        o = default_options(**opts)
        m = max(M, 1)
        qo, to = np.zeros((m, n, 4)), np.zeros((m, n, 3))
        picked = np.full((m, n), -1, dtype=np.intc)
        s = (Summary * (m * n))() if summaries else None
        best = np.zeros(n, dtype=np.intc)
        _check(load().ea_batch_search_starts(self._h, K, _dp(q), _dp(t), M, C.byref(o), _dp(qo), _dp(to),
                                             picked.ctypes.data_as(C.POINTER(C.c_int)), s, best.ctypes.data_as(C.POINTER(C.c_int))))
        self._resident_K = K
        out = [[summary_to_dict(s[k * n + i]) for i in range(n)] for k in range(m)] if summaries else None
        return qo, to, picked.astype(np.int64), out, best.astype(np.int64)

    def bench_resident_poses(self, reps, evaluations_only=False):
        """(ms per run of the resident poses' launches -- one event pair on the batch's stream around `reps` runs --,
        evaluation launches per run); evaluations_only: without the fold launches"""
        ms, n = C.c_double(), C.c_int()
        _check(load().ea_batch_bench_resident_poses(self._h, int(reps), int(evaluations_only), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def solve(self, q, t, **opts):
        q = _f64(q).reshape(-1, 4).copy()
        t = _f64(t).reshape(-1, 3).copy()
        o = default_options(**opts)
        s = (Summary * len(self))()
        _check(load().ea_batch_solve(self._h, C.byref(o), _dp(q), _dp(t), s))
        return q, t, [summary_to_dict(x) for x in s]

    def solve_starts(self, q, t, summaries=True, **opts):
        """K solves of every problem from K starting poses in lock-step (ea_batch_solve_starts): q (K, n, 4), t (K, n, 3)
        -> (q (K, n, 4), t (K, n, 3), K lists of n summaries (None with summaries=False), best (n,))"""
        n = len(self)
        q, t = _f64(q).reshape(-1, n, 4).copy(), _f64(t).reshape(-1, n, 3).copy()
        K = q.shape[0]
        assert t.shape[0] == K
        o = default_options(**opts)
        s = (Summary * (K * n))() if summaries else None
        best = np.zeros(n, dtype=np.intc)
        _check(load().ea_batch_solve_starts(self._h, K, C.byref(o), _dp(q), _dp(t), s, best.ctypes.data_as(C.POINTER(C.c_int))))
        out = [[summary_to_dict(s[k * n + i]) for i in range(n)] for k in range(K)] if summaries else None
        return q, t, out, best.astype(np.int64)

    def bench_eval(self, q, t, warmup, steps, kernel_pass=True):
        """(ms over `steps` fused evaluations, mean ms of the per-point kernel alone | None)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        ms_total, ms_kernel = C.c_double(), C.c_double()
        _check(load().ea_batch_bench_eval(self._h, _dp(q), _dp(t), warmup, steps, C.byref(ms_total),
                                          C.byref(ms_kernel) if kernel_pass else None))
        return ms_total.value, (ms_kernel.value if kernel_pass else None)

    def bench_capture(self, steps):
        """untimed: capture `steps` steps into a hipGraph that bench_steps(steps) replays"""
        _check(load().ea_batch_bench_capture(self._h, int(steps)))

    def bench_capture_pipelined(self, steps):
        """untimed: the same steps with the fold of step k-1 riding in the launch of evaluation k (K launches + 1)"""
        _check(load().ea_batch_bench_capture_pipelined(self._h, int(steps)))

    def bench_result(self, riding=False):
        """what the last step of the last bench_steps left in the batch's result array (layout of eval);
        riding=True: the last-but-one step's result of a pipelined sequence (folded inside an evaluation launch)"""
        n = len(self)
        cost, JtJ, Jtr = np.zeros(n), np.zeros((n, 6, 6)), np.zeros((n, 6))
        bad = np.zeros(n, dtype=np.int64)
        fn = load().ea_batch_bench_result_riding if riding else load().ea_batch_bench_result
        _check(fn(self._h, _dp(cost), _dp(JtJ), _dp(Jtr), bad.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(cost=cost, JtJ=JtJ, Jtr=Jtr, n_invalid=bad)

    def bench_steps(self, steps, host_times=False, riding=False):
        """`steps` x (fused evaluation + fold) at the poses already on the device, then a stream sync: the timed region.
        riding=True: launch by launch with the fold of step k-1 riding in evaluation k (no graph)"""
        fn = load().ea_batch_bench_steps_riding if riding else load().ea_batch_bench_steps
        if host_times:
            us = np.zeros(3)
            _check(fn(self._h, int(steps), _dp(us)))
            return us
        _check(fn(self._h, int(steps), None))

    def bench_kernel(self, q, t, warmup, launches):
        """mean ms of the per-point kernel over `launches` back-to-back launches (one event pair)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        ms = C.c_double()
        _check(load().ea_batch_bench_kernel(self._h, _dp(q), _dp(t), warmup, launches, C.byref(ms)))
        return ms.value

    def row_offsets(self):
        """rows of problem i in the materialised outputs: [offsets[i], offsets[i + 1])"""
        off = np.zeros(len(self) + 1, dtype=np.int64)
        _check(load().ea_batch_row_offsets(self._h, off.ctypes.data_as(C.POINTER(C.c_int64))))
        return off

    def eval_rows(self, q, t, corrected=True, layout=0):
        """materialised mode into host arrays of the batch's dtype: r [rows], J [rows, 6] (layout 0) or [6, rows] (layout 1)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        n = int(self.row_offsets()[-1])
        dt = np.float32 if self.dtype == EA_F32 else np.float64
        r = np.zeros(n, dtype=dt)
        J = np.zeros((n, 6) if layout == 0 else (6, n), dtype=dt)
        bad = C.c_int64()
        _check(load().ea_batch_eval_rows(self._h, _dp(q), _dp(t), int(corrected), int(layout), r.ctypes.data_as(C.c_void_p),
                                         J.ctypes.data_as(C.c_void_p), n, C.byref(bad)))
        return r, J, bad.value

    def eval_rows_device(self, q, t, r_ptr, J_ptr, capacity_rows=None, corrected=True, layout=0):
        """materialised mode into the caller's device arrays; returns n_invalid.  r_ptr / J_ptr: torch tensors on the batch's
        GPU (checked here: device, dtype, contiguity, size) or raw device addresses (then capacity_rows is required and
        the addresses are taken on trust)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        if hasattr(r_ptr, "data_ptr") or hasattr(J_ptr, "data_ptr"):
            import torch
            want = torch.float32 if self.dtype == EA_F32 else torch.float64
            rows = None
            for name, x, per_row in (("r", r_ptr, 1), ("J", J_ptr, 6)):
                if not hasattr(x, "data_ptr"):
                    raise TypeError("%s: pass torch tensors for both outputs or raw addresses for both" % name)
                if not x.is_cuda or x.dtype != want or not x.is_contiguous():
                    raise ValueError("%s must be a contiguous %s tensor on the batch's GPU" % (name, want))
                if x.device.index is not None and x.device.index != self.problems[0].device:
                    raise ValueError("%s lives on cuda:%d, the batch on device %d" % (name, x.device.index, self.problems[0].device))
                n = x.numel() // per_row
                rows = n if rows is None else min(rows, n)
            capacity_rows = rows if capacity_rows is None else min(int(capacity_rows), rows)
            torch.cuda.current_stream(r_ptr.device).synchronize()   # the tensors' producers are done before the library writes
            r_ptr, J_ptr = r_ptr.data_ptr(), J_ptr.data_ptr()
        if capacity_rows is None:
            raise ValueError("capacity_rows is required with raw addresses")
        bad = C.c_int64()
        _check(load().ea_batch_eval_rows_device(self._h, _dp(q), _dp(t), int(corrected), int(layout), C.c_void_p(r_ptr),
                                                C.c_void_p(J_ptr), int(capacity_rows), C.byref(bad)))
        return bad.value

    def bench_rows(self, q, t, warmup, launches, corrected=True, layout=0, mode=1, r_ptr=None, J_ptr=None, capacity_rows=0):
        """mean ms of the materialised-mode kernel over `launches` back-to-back launches (one event pair)"""
        q, t = _f64(q).reshape(-1, 4), _f64(t).reshape(-1, 3)
        ms = C.c_double()
        _check(load().ea_batch_bench_rows(self._h, _dp(q), _dp(t), int(corrected), int(layout), int(mode),
                                          C.c_void_p(r_ptr) if r_ptr else None, C.c_void_p(J_ptr) if J_ptr else None,
                                          int(capacity_rows), warmup, launches, C.byref(ms)))
        return ms.value

    def bench_fold(self, warmup, launches):
        """mean ms of the fold kernel over `launches` back-to-back launches (one event pair)"""
        ms = C.c_double()
        _check(load().ea_batch_bench_fold(self._h, warmup, launches, C.byref(ms)))
        return ms.value

    def set_tuning(self, key, value):
        _check(load().ea_batch_set_tuning(self._h, key.encode(), int(value)))

    def info(self, key):
        v = C.c_int64()
        _check(load().ea_batch_get_info(self._h, key.encode(), C.byref(v)))
        return v.value


def resize_half(img, nan_to_zero=False, device=0):
    """cv::resize(img, dst, Size(), 0.5, 0.5) on the device (ea_resize_half): uint8 H x W x 3 or float32 H x W"""
    img = np.ascontiguousarray(img)
    if img.dtype == np.uint8:
        assert img.ndim == 3 and img.shape[2] == 3
        kind, out = 0, np.zeros((img.shape[0] // 2, img.shape[1] // 2, 3), np.uint8)
    else:
        img = np.ascontiguousarray(img, dtype=np.float32)
        assert img.ndim == 2
        kind, out = (1 if nan_to_zero else 2), np.zeros((img.shape[0] // 2, img.shape[1] // 2), np.float32)
    _check(load().ea_resize_half(device, kind, img.ctypes.data_as(C.c_void_p), img.shape[0], img.shape[1],
                                 out.ctypes.data_as(C.c_void_p)))
    return out


def resize_half_levels(img, skip=0, keep=1, nan_to_zero=False, device=0):
    """ea_resize_half_levels: levels skip .. skip + keep - 1 of the halving chain of img (level k = k halvings, level 0 the frame
    itself) -> list of arrays; img and nan_to_zero as for resize_half (NaN is replaced on the first step only)"""
    img = np.ascontiguousarray(img)
    if img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3:
        kind = 0
    elif img.dtype == np.float32 and img.ndim == 2:
        kind = 1 if nan_to_zero else 2
    else:
        raise ValueError("resize_half_levels takes uint8 (H, W, 3) or float32 (H, W)")
    H, W = img.shape[:2]
    out = [np.empty((H >> k, W >> k) + img.shape[2:], dtype=img.dtype) for k in range(skip, skip + max(keep, 0))] if skip >= 0 else []
    ptrs = (C.c_void_p * max(len(out), 1))(*[o.ctypes.data for o in out])
    _check(load().ea_resize_half_levels(device, kind, img.ctypes.data_as(C.c_void_p), H, W, int(skip), int(keep), ptrs))
    return out


def set_frames_ros_pyramid(levels, ref_bgr=None, ref_depth=None, now_bgr=None, t1=150.0, t2=100.0, halvings=0):
    """ea_batch_set_frames_ros_pyramid[_device]: levels = [Batch of the same N frame pairs' problems per pyramid level], levels[0]
    the finest at the frames' extent >> halvings; every level ends as Batch.set_frames_ros(..., halvings=halvings + l) leaves it,
    bit for bit, from frames that go up once.  The frames as for Batch.set_frames_ros.  A current frame without an edge at some
    level raises EAError(EA_ERR_STATE) after everything else has been set: levels[l].info("frames_without_edges")."""
    sides = [("ref_bgr", ref_bgr, 3), ("ref_depth", ref_depth, 4), ("now_bgr", now_bgr, 3)]
    if (ref_bgr is None) != (ref_depth is None) or all(v is None for _, v, _ in sides):
        raise ValueError("ref_bgr and ref_depth go together, and one side must be given")
    levels = list(levels)
    if not levels:
        raise EAError(EA_ERR_INVALID_ARG, "a pyramid has at least one level")
    shape, on_device, arrays, keep = levels[0]._frame_arrays(sides)
    L = load()
    prm = RosFrameParams()
    L.ea_default_ros_frame_params(C.byref(prm), *(shape or (0, 0)))
    prm.halvings, prm.threshold1, prm.threshold2 = int(halvings), float(t1), float(t2)
    if on_device:
        import torch
        torch.cuda.current_stream(levels[0].problems[0].device).synchronize()  # (as in Batch.set_frames)
    hs = (C.c_void_p * len(levels))(*[b._h for b in levels])
    fn = L.ea_batch_set_frames_ros_pyramid_device if on_device else L.ea_batch_set_frames_ros_pyramid
    _check(fn(hs, len(levels), arrays["ref_bgr"], arrays["ref_depth"], arrays["now_bgr"], C.byref(prm)))


def solve_pyramid_batch(levels, q, t, **opts):
    """ea_batch_solve_pyramid: solve_pyramid for every problem of the levels' batches (levels[0] = finest), one batch solve per
    level; q (N, 4), t (N, 3) -> q, t, [[summary per problem] per level]"""
    levels = list(levels)
    n = len(levels[0]) if levels else 0
    q, t = _f64(q).reshape(-1, 4).copy(), _f64(t).reshape(-1, 3).copy()
    o = default_options(**opts)
    hs = (C.c_void_p * max(len(levels), 1))(*[b._h for b in levels])
    s = (Summary * max(len(levels) * n, 1))()
    _check(load().ea_batch_solve_pyramid(hs, len(levels), C.byref(o), _dp(q), _dp(t), s))
    return q, t, [[summary_to_dict(s[l * n + i]) for i in range(n)] for l in range(len(levels))]


def selftest_wave_reduce(values, device=0):
    """values: (32, 64) float32 -> (totals from the fp32 reduction, totals from the fp64 reduction, stages (30,64))"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    assert v.shape == (32, 64)
    o32, o64 = np.zeros(32), np.zeros(32)
    st = np.zeros((30, 64), dtype=np.float32)
    _check(load().ea_selftest_wave_reduce(device, v.ctypes.data_as(C.POINTER(C.c_float)), _dp(o32), _dp(o64),
                                          st.ctypes.data_as(C.POINTER(C.c_float))))
    return o32, o64, st


def selftest_select(values, offsets, probs, device=0):
    """the select kernels on caller-supplied doubles: segment s = values[offsets[s]:offsets[s + 1]], NaN = failed block,
    everything else by absolute value -> (out [nseg, len(probs)], n_valid [nseg])"""
    v, probs = _f64(values).reshape(-1), _f64(probs).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    nseg = off.size - 1
    out, m = np.zeros((nseg, probs.size)), np.zeros(nseg, dtype=np.int64)
    _check(load().ea_selftest_select(device, _dp(v), off.ctypes.data_as(C.POINTER(C.c_int64)), nseg, _dp(probs), probs.size,
                                     _dp(out), m.ctypes.data_as(C.POINTER(C.c_int64))))
    return out, m
