"""ctypes binding of include/city2ba_hip.h (the C-ABI shared library built from csrc/).

There is NO CPU fallback: if the HIP library is missing this module raises at import of the
first symbol, and every compute entry point fails with C2B_ERR_NO_DEVICE when no GPU is visible.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcity2ba_hip.so")

OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_INDEX_OUT_OF_RANGE = -2
ERR_HIP = -3
ERR_OOM = -4
ERR_NO_DEVICE = -5
ERR_RCCL = -6
COMM_ID_BYTES = 128
ABI_VERSION = 10           # include/city2ba_hip.h: C2B_ABI_VERSION
CAMBLK_DOUBLES = 32
STATS_DOUBLES = 20

_vp = C.c_void_p
_i64 = C.c_int64
_u64 = C.c_uint64
_d = C.c_double
_int = C.c_int


# robust losses of the step (c2b_problem_set_loss): name -> kind; None and "squared" are the squared loss
LOSS_KINDS = {None: 0, "squared": 0, "huber": 1, "cauchy": 2, "soft_l1": 3}
LOSS_NAMES = {0: None, 1: "huber", 2: "cauchy", 3: "soft_l1"}


def loss_kind(loss):
    """the C ABI's kind of a loss given by name (or None, or the kind itself)"""
    if isinstance(loss, int) and not isinstance(loss, bool):
        return loss
    try:
        return LOSS_KINDS[loss]
    except (KeyError, TypeError):
        raise ValueError("loss must be None, 'huber', 'cauchy' or 'soft_l1', not %r" % (loss,))


# preconditioners of the step's PCG (c2b_problem_set_preconditioner): name -> kind
PRECOND_KINDS = {"block_jacobi": 0, "schur_jacobi": 1}
PRECOND_NAMES = {0: "block_jacobi", 1: "schur_jacobi"}


def precond_kind(name):
    """the C ABI's kind of a preconditioner given by name (or the kind itself)"""
    if isinstance(name, int) and not isinstance(name, bool):
        return name
    try:
        return PRECOND_KINDS[name]
    except (KeyError, TypeError):
        raise ValueError("preconditioner must be 'block_jacobi' or 'schur_jacobi', not %r" % (name,))


# how the step applies the Schur complement (c2b_problem_set_schur): name -> kind
SCHUR_KINDS = {"implicit": 0, "explicit": 1}
SCHUR_NAMES = {0: "implicit", 1: "explicit"}


def schur_kind(name):
    """the C ABI's kind of a Schur complement given by name (or the kind itself)"""
    if isinstance(name, int) and not isinstance(name, bool):
        return name
    try:
        return SCHUR_KINDS[name]
    except (KeyError, TypeError):
        raise ValueError("schur must be 'implicit' or 'explicit', not %r" % (name,))


# how the step solves the reduced camera system (c2b_problem_set_linear_solver): name -> kind
LINEAR_KINDS = {"pcg": 0, "cholesky": 1}
LINEAR_NAMES = {0: "pcg", 1: "cholesky"}
DENSE_MAX_CAMERAS = 4096    # C2B_DENSE_MAX_CAMERAS: the direct solve refuses more cameras than this


def linear_kind(name):
    """the C ABI's kind of a linear solver given by name (or the kind itself)"""
    if isinstance(name, int) and not isinstance(name, bool):
        return name
    try:
        return LINEAR_KINDS[name]
    except (KeyError, TypeError):
        raise ValueError("linear_solver must be 'pcg' or 'cholesky', not %r" % (name,))


class StepInfo(C.Structure):
    """c2b_step_info (include/city2ba_hip_experimental.h)"""
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("rel_residual", C.c_double), ("sum_sq", C.c_double),
                ("model_decrease", C.c_double)]


class LmOptions(C.Structure):
    """c2b_lm_options (include/city2ba_hip_experimental.h)"""
    _fields_ = [("max_iterations", C.c_int32), ("pcg_max_iters", C.c_int32), ("lambda0", C.c_double), ("pcg_rel_tol", C.c_double),
                ("function_tol", C.c_double), ("gradient_tol", C.c_double), ("parameter_tol", C.c_double)]


class RefineOptions(C.Structure):
    """c2b_refine_options (include/city2ba_hip_experimental.h)"""
    _fields_ = [("max_rounds", C.c_int32), ("reserved", C.c_int32), ("lambda0", C.c_double), ("function_tol", C.c_double),
                ("gradient_tol", C.c_double), ("parameter_tol", C.c_double)]


class LmIteration(C.Structure):
    """c2b_lm_iteration"""
    _fields_ = [("cost", C.c_double), ("cost_trial", C.c_double), ("lam", C.c_double), ("model_decrease", C.c_double),
                ("gradient_max", C.c_double), ("step_norm", C.c_double), ("x_norm", C.c_double), ("pcg_rel_residual", C.c_double),
                ("accepted", C.c_int32), ("pcg_iterations", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class LmSummary(C.Structure):
    """c2b_lm_summary"""
    _fields_ = [("iterations", C.c_int32), ("termination", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("lambda_next", C.c_double)]


class Similarity(C.Structure):
    """c2b_similarity (include/city2ba_hip_experimental.h): y = scale * rotation x + translation, rotation row-major"""
    _fields_ = [("scale", C.c_double), ("rotation", C.c_double * 9), ("translation", C.c_double * 3)]


class AlignOptions(C.Structure):
    """c2b_align_options"""
    _fields_ = [("on", C.c_int32), ("scale", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32), ("max_dist", C.c_double),
                ("use_cam", C.c_void_p), ("use_pt", C.c_void_p)]


class AlignStat(C.Structure):
    """c2b_align_stat"""
    _fields_ = [("n", C.c_int64), ("argmax", C.c_int64), ("sum_sq", C.c_double), ("sum", C.c_double), ("max", C.c_double)]


class AlignSummary(C.Structure):
    """c2b_align_summary"""
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("cameras", AlignStat), ("camera_rotations", AlignStat), ("points", AlignStat)]


# c2b_align_options.on (C2B_ALIGN_CAMERAS / _POINTS / _BOTH) and c2b_align_summary.status (C2B_ALIGN_OK / _TOO_FEW / _DEGENERATE)
ALIGN_ON = {"cameras": 1, "points": 2, "both": 3}
ALIGN_OK, ALIGN_TOO_FEW, ALIGN_DEGENERATE = range(3)
ALIGN_STATUS = ("ok", "too_few", "degenerate")

# c2b_lm_summary.termination
LM_TERMINATIONS = {0: "max_iterations", 1: "function_tolerance", 2: "gradient_tolerance", 3: "parameter_tolerance", 4: "not_finite"}


# flags of c2b_problem_filter_observations / c2b_residual_keep_rows
FILTER_IN_FRONT = 1        # C2B_FILTER_IN_FRONT: also drop an observation whose point is not in front of its camera

# statuses of c2b_problem_triangulate_points / c2b_triangulate_rows (C2B_TRI_*), the order of their counts
TRI_OK, TRI_TOO_FEW, TRI_DEGENERATE, TRI_BEHIND, TRI_CONSTANT = range(5)
TRI_STATUS = ("triangulated", "too_few", "degenerate", "behind", "constant")
# c2b_problem_triangulate_consensus / c2b_triangulate_consensus_rows add one status (C2B_TRI_NO_CONSENSUS) and one flag
TRI_NO_CONSENSUS = 5
TRI_CONSENSUS_STATUS = TRI_STATUS + ("no_consensus",)
TRI_DROP_OUTLIERS = 1      # C2B_TRI_DROP_OUTLIERS: compact the list by the inlier mask afterwards

# statuses of c2b_problem_refine_points / c2b_refine_points_rows (C2B_REFINE_*); their counts hold one more entry, `moved`
REFINE_CONVERGED, REFINE_MAX_ROUNDS, REFINE_UNOBSERVED, REFINE_FAILED, REFINE_CONSTANT = range(5)
REFINE_STATUS = ("converged", "max_rounds", "unobserved", "failed", "constant")
REFINE_COUNTS = REFINE_STATUS + ("moved",)

# statuses of c2b_problem_resect_cameras / c2b_resect_rows (C2B_RES_*), the order of their counts
RES_OK, RES_TOO_FEW, RES_DEGENERATE, RES_BEHIND, RES_CONSTANT = range(5)
RES_STATUS = ("resected", "too_few", "degenerate", "behind", "constant")
# c2b_problem_resect_consensus / c2b_resect_consensus_rows add one status (C2B_RES_NO_CONSENSUS) and one flag
RES_NO_CONSENSUS = 5
RES_CONSENSUS_STATUS = RES_STATUS + ("no_consensus",)
RES_DROP_OUTLIERS = 1      # C2B_RES_DROP_OUTLIERS: compact the list by the inlier mask afterwards

# statuses of c2b_merge_partner_rows (C2B_MERGE_*), the order of its counts
MERGE_NONE, MERGE_CHOSEN, MERGE_UNOBSERVED, MERGE_HELD = range(4)
MERGE_STATUS = ("none", "chosen", "unobserved", "held")

# statuses of c2b_rematch_rows (C2B_REMATCH_*), the order of its counts
REMATCH_FITS, REMATCH_SKIPPED, REMATCH_REASSIGNED, REMATCH_REMOVED = range(4)
REMATCH_STATUS = ("fits", "skipped", "reassigned", "removed")

# flags of c2b_problem_subset / c2b_problem_window
SUBSET_CARRY = 1           # C2B_SUBSET_CARRY: the child takes the parent's handle state and, for repeat-free lists, an origin
WINDOW_HALO = 1            # C2B_WINDOW_HALO: halo cameras held constant; 0 = no halo cameras, shared points held constant

# c2b_covisibility_temp_bytes' passes (C2B_COVIS_TEMP_*)
COVIS_TEMP_GRAPH, COVIS_TEMP_EXPAND = 0, 1


# name -> (restype, argtypes).  Kept in one table so tests can check every symbol the header declares.
SIGNATURES = {
    "c2b_version": (C.c_char_p, []),
    "c2b_abi_version": (_int, []),
    "c2b_last_error": (C.c_char_p, []),
    "c2b_device_count": (_int, [C.POINTER(_int)]),
    "c2b_workspace_bytes": (_i64, [_i64]),
    "c2b_workspace_init": (_int, [_vp, _vp]),
    "c2b_workspace_selfcheck": (_int, [_vp, _vp, C.POINTER(_i64)]),
    "c2b_cameras_from_bal": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_cameras_to_bal": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_camblk_doubles": (_i64, [_i64]),
    "c2b_camblk_from_state": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "c2b_camblk_from_bal": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "c2b_cameras_from_position_direction": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "c2b_project_world": (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "c2b_to_world": (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "c2b_cameras_transform": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "c2b_points_pad": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_points_unpad": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_expand_rows": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "c2b_project": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "c2b_reprojection_error_sum": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
    "c2b_rows_tiles_bytes": (_i64, [_i64]),
    "c2b_rows_pack": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "c2b_project_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "c2b_reprojection_error_sum_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
    "c2b_visibility_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
    "c2b_visibility_rows_bits": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
    "c2b_residual_keep_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _d, _int, _vp, _vp]),
    "c2b_triangulate_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp]),
    "c2b_refine_points_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_refine_cameras_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _int, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_triangulate_consensus_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _d, _d, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_resect_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _int, _d, _vp, _vp, _vp, _vp]),
    "c2b_resect_consensus_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _d, _int, _d, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_merge_partner_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "c2b_rematch_rows": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _d, _d, _vp, _vp, _vp, _vp]),
    "c2b_reprojection_error_sums2_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "c2b_add_noise_observations_error_sums2_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _d, _u64, _vp, _vp, _vp]),
    "c2b_jacobian_stream_policy": (_int, [_i64, _i64, _i64]),
    "c2b_jacobian_tiles_per_wave": (_int, [_i64]),
    "c2b_jacobian_launch_shape": (_int, [_i64, _d, _vp, _vp]),
    "c2b_jacobian_outputs_store_rate": (_int, [_vp, _vp]),
    "c2b_jacobian_outputs_set_store_rate": (_int, [_vp, _d]),
    "c2b_residual_jacobian_rows_placed": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _d, _vp, _vp, _vp]),
    "c2b_residual_jacobian_rows": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _d, _vp, _vp, _vp]),
    "c2b_residual_jacobian": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _d, _vp, _vp]),
    "c2b_error_sum_finish": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_residual_jacobian_sum": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _d, _vp, _vp, _vp]),
    "c2b_host_alloc": (_int, [C.POINTER(_vp), _i64]),
    "c2b_host_free": (None, [_vp]),
    "c2b_jacobian_outputs_alloc": (_int, [_i64, _int, _d, _vp, C.POINTER(_vp)]),
    "c2b_jacobian_outputs_pointers": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "c2b_jacobian_outputs_log": (_int, [_vp, _vp, _int, C.POINTER(_int), C.POINTER(_int)]),
    "c2b_jacobian_outputs_free": (None, [_vp]),
    "c2b_calib_store_pattern": (_int, [_i64, _vp, _vp, _vp, _vp]),
    "c2b_calib_copy": (_int, [_vp, _vp, _i64, _vp]),
    "c2b_normal_transpose_temp_bytes": (_i64, [_i64, _i64]),
    "c2b_normal_transpose": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "c2b_normal_cameras_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "c2b_normal_points_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_schur_points_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp]),
    "c2b_schur_cameras_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _d, _vp, _vp, _vp, _vp]),
    "c2b_problem_solve_step": (_int, [_vp, _d, _int, _d, _vp, _vp, _vp]),
    "c2b_problem_apply_step": (_int, [_vp, _vp, _vp]),
    "c2b_problem_checkpoint": (_int, [_vp]),
    "c2b_problem_rollback": (_int, [_vp]),
    "c2b_problem_drop_checkpoint": (_int, [_vp]),
    "c2b_problem_levenberg_marquardt": (_int, [_vp, _vp, _vp, _int, _vp]),
    "c2b_problem_filter_observations": (_int, [_vp, _d, _int, C.POINTER(_i64)]),
    "c2b_problem_triangulate_points": (_int, [_vp, _d, _vp, _vp]),
    "c2b_problem_refine_points": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_problem_refine_cameras": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_problem_set_inner_iterations": (_int, [_vp, _int]),
    "c2b_problem_get_inner_iterations": (_int, [_vp, C.POINTER(_int)]),
    "c2b_problem_triangulate_consensus": (_int, [_vp, _d, _d, _int, _int, _int, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "c2b_problem_resect_cameras": (_int, [_vp, _int, _d, _vp, _vp]),
    "c2b_problem_resect_consensus": (_int, [_vp, _d, _int, _d, _int, _int, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "c2b_problem_merge_points": (_int, [_vp, _d, _d, _int, _vp, C.POINTER(_i64), C.POINTER(_int)]),
    "c2b_problem_rematch_observations": (_int, [_vp, _d, _d, _int, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_drop_keep_rows": (_int, [_vp, _i64, _i64, _d, _u64, _vp, _vp]),
    "c2b_mismatch_partner_rows": (_int, [_vp, _i64, _vp, _i64, _d, _u64, _vp, _vp, _vp]),
    "c2b_select_smallest_keys_rows": (_int, [_vp, _i64, _u64, _int, _int, _i64, _vp, _vp]),
    "c2b_nearest_points_rows": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "c2b_problem_drop_features": (_int, [_vp, _d, _u64, C.POINTER(_i64)]),
    "c2b_problem_add_incorrect_correspondences": (_int, [_vp, _d, _u64, C.POINTER(_i64)]),
    "c2b_problem_split_landmarks": (_int, [_vp, _d, _u64, C.POINTER(_i64)]),
    "c2b_problem_join_landmarks": (_int, [_vp, _d, _u64, C.POINTER(_i64)]),
    "c2b_problem_subset": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _vp]),
    "c2b_problem_window": (_int, [_vp, _vp, _int, _vp]),
    "c2b_problem_get_origin": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_write_back": (_int, [_vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_covisibility_temp_bytes": (_i64, [_i64, _int]),
    "c2b_covisibility_degree_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "c2b_covisibility_fill_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "c2b_covisibility_expand_rows": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_covisibility": (_int, [_vp, _int, C.POINTER(_i64)]),
    "c2b_problem_get_covisibility": (_int, [_vp, _vp, _vp, _vp, C.POINTER(_int), C.POINTER(_i64)]),
    "c2b_problem_neighbourhood": (_int, [_vp, _vp, _int, _int, _i64, _vp, _vp, _vp, C.POINTER(_i64)]),
    "c2b_problem_set_loss": (_int, [_vp, _int, _d]),
    "c2b_problem_get_loss": (_int, [_vp, C.POINTER(_int), C.POINTER(_d)]),
    "c2b_problem_robust_cost": (_int, [_vp, C.POINTER(_d)]),
    "c2b_normal_cameras_rows_loss": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _d, _vp]),
    "c2b_normal_points_rows_loss": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _d, _vp]),
    "c2b_schur_points_rows_loss": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _int, _d, _vp]),
    "c2b_schur_cameras_rows_loss": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _d, _vp, _vp, _vp, _int, _d, _vp]),
    "c2b_problem_set_preconditioner": (_int, [_vp, _int]),
    "c2b_problem_get_preconditioner": (_int, [_vp, C.POINTER(_int)]),
    "c2b_problem_preconditioner_fallbacks": (_int, [_vp, C.POINTER(_i64)]),
    "c2b_problem_set_schur": (_int, [_vp, _int]),
    "c2b_problem_get_schur": (_int, [_vp, C.POINTER(_int)]),
    "c2b_problem_schur_bytes": (_int, [_vp, C.POINTER(_i64)]),
    "c2b_problem_schur_complement": (_int, [_vp, _d, _vp, _vp, _vp, C.POINTER(_i64)]),
    "c2b_problem_get_schur_pattern": (_int, [_vp, _vp, _vp]),
    "c2b_schur_y_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _d, _vp, _vp]),
    "c2b_schur_y_rows_loss": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _d, _vp, _int, _d, _vp]),
    "c2b_schur_blocks_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_schur_spmv_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_set_linear_solver": (_int, [_vp, _int]),
    "c2b_problem_get_linear_solver": (_int, [_vp, C.POINTER(_int)]),
    "c2b_problem_linear_solver_bytes": (_int, [_vp, C.POINTER(_i64)]),
    "c2b_dense_scatter_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "c2b_dense_cholesky": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "c2b_dense_cholesky_solve": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "c2b_problem_set_constant": (_int, [_vp, _vp, _vp]),
    "c2b_problem_get_constant": (_int, [_vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_problem_set_priors": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_get_priors": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_problem_prior_cost": (_int, [_vp, C.POINTER(_d)]),
    "c2b_problem_prior_residual_jacobian": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_prior_cameras_rows": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_prior_points_rows": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_prior_model_rows": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_schur_jacobi_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _d, _vp, _vp]),
    "c2b_schur_jacobi_rows_loss": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _d, _vp, _int, _d, _vp]),
    "c2b_visibility_pairs": (_int, [_vp, _vp, _vp, _vp, _i64, _d, _vp, _vp, _vp]),
    "c2b_visibility_dense_tiles": (_i64, [_i64]),
    "c2b_visibility_dense_count": (_int, [_vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp]),
    "c2b_visibility_dense_fill": (_int, [_vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp, _vp]),
    "c2b_occlusion_filter": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "c2b_bvh_build": (_int, [_vp, _i64, C.POINTER(_vp)]),
    "c2b_bvh_sizes": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_int)]),
    "c2b_bvh_copy": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_bvh_free": (None, [_vp]),
    "c2b_occlusion_filter_bvh": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "c2b_stats": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "c2b_stats_partial_pass1": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "c2b_stats_partial_pass2": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_stats_combine_shares": (_int, [_vp, _int, _vp]),
    "c2b_stats_finish_shares": (_int, [_vp, _int, _i64, _vp]),
    "c2b_comm_backend": (C.c_char_p, []),
    "c2b_comm_unique_id": (_int, [_vp]),
    "c2b_comm_init_rank": (_int, [_vp, _int, _int, _int, C.POINTER(_vp)]),
    "c2b_comm_init_all": (_int, [_int, _vp, _vp]),
    "c2b_comm_group_start": (_int, []),
    "c2b_comm_group_end": (_int, []),
    "c2b_comm_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "c2b_comm_all_reduce_sum_f64": (_int, [_vp, _vp, _i64, _vp]),
    "c2b_comm_all_gather_f64": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "c2b_comm_destroy": (None, [_vp]),
    "c2b_stats_sharded": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "c2b_add_drift_sharded": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _int, _d, _d, _d, _d, _d, _d, _u64, _vp]),
    "c2b_add_noise_entities_sharded": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _d, _d, _d, _u64, _vp]),
    "c2b_add_drift": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _d, _d, _d, _u64, _vp]),
    "c2b_add_drift_normalized": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _u64, _vp]),
    "c2b_add_noise_entities": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _u64, _vp]),
    "c2b_add_noise_observations": (_int, [_vp, _i64, _i64, _d, _u64, _vp]),
    "c2b_add_sin_noise": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _d, _d, _d, _d, _d, _vp]),
    "c2b_convert_f64_to_f32": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_convert_f32_to_f64": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_stats_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "c2b_add_drift_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _d, _d, _d, _u64, _vp]),
    "c2b_add_drift_normalized_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _u64, _vp]),
    "c2b_add_noise_entities_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _u64, _vp]),
    "c2b_add_sin_noise_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _d, _d, _d, _d, _d, _d, _d, _d, _vp]),
    "c2b_partition_cameras": (_int, [_vp, _i64, _int, _vp]),
    "c2b_synthetic_grid_sizes": (_int, [_i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_synthetic_grid_layout": (_int, [_i64, _i64, _i64, _d, _d, _d, _d, _vp, _vp, _vp]),
    "c2b_synthetic_line_layout": (_int, [_i64, _i64, _d, _d, _d, _d, _vp, _vp, _vp]),
    "c2b_candidate_pairs": (_int, [_vp, _i64, _vp, _i64, _d, _i64, _i64, _int, _d, _d, _int, C.POINTER(_vp)]),
    "c2b_pairs_count": (_i64, [_vp]),
    "c2b_pairs_cam_idx": (_vp, [_vp]),
    "c2b_pairs_pt_idx": (_vp, [_vp]),
    "c2b_pairs_free": (None, [_vp]),
    "c2b_obj_load": (_int, [C.c_char_p, C.POINTER(_vp)]),
    "c2b_obj_model_count": (_i64, [_vp]),
    "c2b_obj_model_name": (C.c_char_p, [_vp, _i64]),
    "c2b_obj_model_sizes": (_int, [_vp, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_int)]),
    "c2b_obj_model_copy": (_int, [_vp, _i64, _vp, _vp]),
    "c2b_obj_move_to_origin": (_int, [_vp, _i64]),
    "c2b_obj_triangles": (_int, [_vp, _i64, _vp, C.POINTER(_i64)]),
    "c2b_obj_free": (None, [_vp]),
    "c2b_generate_cameras_path": (_int, [_vp, _i64, _i64, _d, _u64, _vp, _vp]),
    "c2b_generate_cameras_poisson": (_int, [_vp, _i64, _i64, _d, _d, _u64, _i64, _vp, _vp, C.POINTER(_i64)]),
    "c2b_generate_cameras_poisson_bvh": (_int, [_vp, _i64, _vp, _i64, _d, _d, _u64, _i64, _vp, _vp, C.POINTER(_i64)]),
    "c2b_modify_intrinsics": (_int, [_vp, _i64, _vp, _vp, _u64]),
    "c2b_generate_world_points": (_int, [_vp, _i64, _vp, _i64, _i64, _d, _u64, _vp, C.POINTER(_i64)]),
    "c2b_cull": (_int, [C.POINTER(_i64), _vp, _int, C.POINTER(_i64), _vp, _vp, _vp, _vp, _int]),
    "c2b_add_incorrect_correspondences": (_int, [_i64, _vp, _vp, _vp, _d, _u64]),
    "c2b_drop_features": (_int, [_i64, _vp, _vp, _vp, _d, _u64]),
    "c2b_split_landmarks": (_int, [C.POINTER(_i64), _vp, _i64, _i64, _vp, _d, _u64]),
    "c2b_join_landmarks": (_int, [_i64, _vp, _i64, _vp, _d, _u64]),
    "c2b_bal_read": (_int, [C.c_char_p, C.POINTER(_vp)]),
    "c2b_bal_sizes": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_bal_copy": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_bal_close": (None, [_vp]),
    "c2b_bal_write": (_int, [C.c_char_p, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_bal_read_as": (_int, [C.c_char_p, _int, C.POINTER(_vp)]),
    "c2b_bal_write_as": (_int, [C.c_char_p, _int, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_format_f64": (_int, [_i64, _vp, _vp, _i64, C.POINTER(_i64)]),
    "c2b_parse_f64": (_int, [C.c_char_p, _i64, _i64, _vp, _vp]),
    "c2b_ply_write": (_int, [C.c_char_p, _i64, _vp, _i64, _vp, _vp, _vp]),
    "c2b_problem_create": (_int, [_int, C.POINTER(_vp)]),
    "c2b_problem_destroy": (None, [_vp]),
    "c2b_problem_options_init": (None, [_vp]),
    "c2b_problem_set_options": (_int, [_vp, _vp]),
    "c2b_problem_get_options": (_int, [_vp, _vp]),
    "c2b_host_set_io_threads": (None, [_int]),
    "c2b_problem_upload": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_problem_upload_bal": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_problem_synthetic_grid_layout": (_int, [_vp, _i64, _i64, _i64, _d, _d, _d, _d]),
    "c2b_problem_synthetic_line_layout": (_int, [_vp, _i64, _i64, _d, _d, _d, _d]),
    "c2b_problem_sizes": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "c2b_problem_download": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_problem_download_bal": (_int, [_vp, _vp]),
    "c2b_problem_write": (_int, [_vp, C.c_char_p, _int]),
    "c2b_problem_read": (_int, [_vp, C.c_char_p, _int]),
    "c2b_problem_from_position_direction": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "c2b_problem_centers": (_int, [_vp, _vp]),
    "c2b_problem_project": (_int, [_vp, _vp]),
    "c2b_problem_total_reprojection_error": (_int, [_vp, _d, C.POINTER(_d)]),
    "c2b_problem_total_reprojection_error_sharded": (_int, [_vp, _vp, _d, C.POINTER(_d)]),
    "c2b_problem_total_reprojection_errors_l1_l2": (_int, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "c2b_problem_total_reprojection_errors_l1_l2_sharded": (_int, [_vp, _vp, C.POINTER(_d), C.POINTER(_d)]),
    "c2b_problem_add_noise_errors_l1_l2": (_int, [_vp, _d, _d, _d, _d, _u64, C.POINTER(_d), C.POINTER(_d)]),
    "c2b_problem_add_noise_errors_l1_l2_sharded": (_int, [_vp, _vp, _d, _d, _d, _d, _u64, C.POINTER(_d), C.POINTER(_d)]),
    "c2b_problem_residual_jacobian": (_int, [_vp, _vp, _vp, _vp]),
    "c2b_problem_residual_jacobian_device": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(_d)]),
    "c2b_problem_normal_equations": (_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_d)]),
    "c2b_problem_stats": (_int, [_vp, _vp]),
    "c2b_problem_visibility_pairs": (_int, [_vp, _i64, _vp, _vp, _d, _vp, _vp]),
    "c2b_problem_cull": (_int, [_vp, _int]),
    "c2b_problem_largest_connected_component": (_int, [_vp, _int]),
    "c2b_problem_remove_singletons": (_int, [_vp]),
    "c2b_largest_connected_component": (_int, [C.POINTER(_i64), _vp, _int, C.POINTER(_i64), _vp, _vp, _vp, _vp, _int]),
    "c2b_remove_singletons": (_int, [C.POINTER(_i64), _vp, _int, C.POINTER(_i64), _vp, _vp, _vp, _vp]),
    "c2b_problem_adopt_visibility": (_int, [_vp]),
    "c2b_problem_download_graph": (_int, [_vp, _vp, _vp]),
    "c2b_problem_export_device": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_visibility_pairs_compact": (_int, [_vp, _i64, _vp, _vp, _d, _vp]),
    "c2b_problem_visibility_within_distance": (_int, [_vp, _d, _int, _d, _d, _vp]),
    "c2b_problem_visibility_dense": (_int, [_vp, _d, _vp]),
    "c2b_problem_visibility_dense_fetch": (_int, [_vp, _vp, _vp]),
    "c2b_problem_visibility_dense_occlude": (_int, [_vp, _vp, _i64, _vp]),
    "c2b_problem_visibility_dense_occlude_bvh": (_int, [_vp, _vp, _vp]),
    "c2b_problem_generate_world_points": (_int, [_vp, _vp, _i64, _i64, _d, _u64, C.POINTER(_i64)]),
    "c2b_problem_add_drift": (_int, [_vp, _d, _d, _d, _vp, _u64]),
    "c2b_problem_add_drift_normalized": (_int, [_vp, _d, _d, _d, _u64]),
    "c2b_problem_add_noise": (_int, [_vp, _d, _d, _d, _d, _u64]),
    "c2b_problem_add_sin_noise": (_int, [_vp, _vp, _vp, _d, _d]),
    "c2b_problem_set_shard": (_int, [_vp, _i64, _i64, _i64]),
    "c2b_align_options_init": (None, [_vp]),
    "c2b_similarity_from_moments": (_int, [_i64, _vp, _vp, _d, _d, _vp, _int, _vp, C.POINTER(_int)]),
    "c2b_align_finish_moments": (_int, [_vp, _vp, C.POINTER(_d), _vp, _vp, C.POINTER(_d), C.POINTER(_d), _vp]),
    "c2b_align_launch_shape": (_int, [C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "c2b_align_means_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "c2b_align_moments_rows": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "c2b_align_errors_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp]),
    "c2b_align_rotation_errors_rows": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_similarity_apply": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "c2b_problem_align": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c2b_problem_transform": (_int, [_vp, _vp]),
    "c2b_problem_stats_sharded": (_int, [_vp, _vp, _vp]),
    "c2b_problem_add_drift_sharded": (_int, [_vp, _vp, _d, _d, _d, _vp, _u64]),
    "c2b_problem_add_noise_sharded": (_int, [_vp, _vp, _d, _d, _d, _d, _u64]),
    "c2b_problem_add_sin_noise_sharded": (_int, [_vp, _vp, _vp, _vp, _d, _d]),
}


class City2baError(RuntimeError):
    """Mirrors the reference's failure modes: bad arguments / the asserts of
    src/baproblem.rs:345-346, 365-369 (status -2) / device errors."""

    def __init__(self, status, message):
        super().__init__("city2ba_hip status %d: %s" % (status, message))
        self.status = status


_lib = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  libcity2ba_hip.so links ROCm's; with
    both loaded a process holds two HIP runtimes and whichever initialises second can fail ("no ROCm-capable
    device", "No HIP GPUs are available") depending on import order.  When torch is installed its runtime is
    therefore opened first, globally, so that this library binds to the same copy torch will use.  Hosts without
    torch (the Rust binding) simply get ROCm's runtime."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "city2ba_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)          # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        if L.c2b_abi_version() != ABI_VERSION:       # the number this table of signatures was written against (C2B_ABI_VERSION)
            raise ImportError("city2ba_amd: %s speaks ABI %d, this binding %d -- rebuild the library" % (LIB_PATH, L.c2b_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(status):
    if status != OK:
        raise City2baError(status, lib().c2b_last_error().decode("utf-8", "replace"))


def similarity(scale, rotation, translation):
    """a c2b_similarity from a scale, a [3, 3] rotation and a [3] translation"""
    import numpy as np
    T = Similarity()
    T.scale = float(scale)
    T.rotation[:] = [float(v) for v in np.asarray(rotation, dtype=np.float64).reshape(9)]
    T.translation[:] = [float(v) for v in np.asarray(translation, dtype=np.float64).reshape(3)]
    return T


def similarity_from_moments(n, mean_x, mean_y, var_x, var_y, cov, scale=True):
    """c2b_similarity_from_moments (host arithmetic, no device): Umeyama's closed form from the centred moments.
    Returns (status, scale, rotation [3, 3], translation [3]); on a failure the identity."""
    import numpy as np
    mx, my, cv = (np.ascontiguousarray(a, dtype=np.float64).reshape(k) for a, k in ((mean_x, 3), (mean_y, 3), (cov, 9)))
    T, st = Similarity(), _int(-1)
    check(lib().c2b_similarity_from_moments(int(n), mx.ctypes.data_as(_vp), my.ctypes.data_as(_vp), float(var_x), float(var_y),
                                            cv.ctypes.data_as(_vp), int(bool(scale)), C.byref(T), C.byref(st)))
    return st.value, T.scale, np.array(T.rotation[:]).reshape(3, 3), np.array(T.translation[:])


def align_finish_moments(means7, moments23):
    """c2b_align_finish_moments (host arithmetic): what the two device passes leave -> dict(n, mean_x, mean_y, var_x, var_y, cov [3, 3])"""
    import numpy as np
    a, b = np.ascontiguousarray(means7, dtype=np.float64).reshape(7), np.ascontiguousarray(moments23, dtype=np.float64).reshape(23)
    n, vx, vy = _d(), _d(), _d()
    mx, my, cov = np.empty(3), np.empty(3), np.empty(9)
    check(lib().c2b_align_finish_moments(a.ctypes.data_as(_vp), b.ctypes.data_as(_vp), C.byref(n), mx.ctypes.data_as(_vp), my.ctypes.data_as(_vp),
                                         C.byref(vx), C.byref(vy), cov.ctypes.data_as(_vp)))
    return dict(n=n.value, mean_x=mx, mean_y=my, var_x=vx.value, var_y=vy.value, cov=cov.reshape(3, 3))


def align_launch_shape():
    """(threads per workgroup, most workgroups, entities per thread and trip) of the alignment passes"""
    a, b, c = _int(), _int(), _int()
    check(lib().c2b_align_launch_shape(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def device_count():
    n = _int(0)
    rc = lib().c2b_device_count(C.byref(n))
    return n.value if rc == OK else 0
