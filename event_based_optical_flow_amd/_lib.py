"""ctypes binding of libcmax_hip.so (the C ABI declared in include/cmax_hip.h).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the shared object cannot
be loaded, or a compute entry point is called without a GPU, this module raises -- loudly.
"""
import ctypes
import os
import threading

from . import build as _build

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_dbl = ctypes.c_double
c_vp = ctypes.c_void_p


class CmaxError(RuntimeError):
    """A libcmax_hip entry point returned non-zero (negative: bad argument, positive: hipError_t)."""

    def __init__(self, code, message):
        super().__init__(f"libcmax_hip error {code}: {message}")
        self.code = code


class CmaxObjective(ctypes.Structure):
    """Mirror of cmax_objective_t (include/cmax_hip.h)."""

    _fields_ = [
        ("model", ctypes.c_int32),
        ("cost", ctypes.c_int32),
        ("normalized", ctypes.c_int32),
        ("minimize", ctypes.c_int32),
        ("negate", ctypes.c_int32),
        ("omit_boundary", ctypes.c_int32),
        ("normalize_t", ctypes.c_int32),
        ("n_ref", ctypes.c_int32),
        ("ref_mode", ctypes.c_int32 * 4),
        ("ref_frac", ctypes.c_double * 4),
        ("mult", ctypes.c_double * 4),
        ("sigma", ctypes.c_double),
        ("T", ctypes.c_int32),
        ("motion_dtype", ctypes.c_int32),
    ]


class CmaxIwes(ctypes.Structure):
    """Mirror of cmax_iwes_t (include/cmax_hip.h)."""

    _fields_ = [
        ("model", ctypes.c_int32),
        ("normalize_t", ctypes.c_int32),
        ("n_ref", ctypes.c_int32),
        ("ref_mode", ctypes.c_int32 * 4),
        ("ref_frac", ctypes.c_double * 4),
        ("sigma", ctypes.c_double),
        ("T", ctypes.c_int32),
        ("motion_dtype", ctypes.c_int32),
        ("with_orig", ctypes.c_int32),
    ]


class CmaxPatchObjective(ctypes.Structure):
    """Mirror of cmax_patch_objective_t (include/cmax_hip.h)."""

    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("time_aware", ctypes.c_int32),
        ("T", ctypes.c_int32),
        ("scheme", ctypes.c_int32),
        ("t0", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("ph", ctypes.c_int32),
        ("pw", ctypes.c_int32),
        ("sw_h", ctypes.c_int32),
        ("sw_w", ctypes.c_int32),
        ("pad_h", ctypes.c_int32),
        ("pad_w", ctypes.c_int32),
        ("tv_omit_boundary", ctypes.c_int32),
        ("scale_later", ctypes.c_int32),
        ("filter_type", ctypes.c_int32),  # the former padding in front of t_scale: the size is unchanged
        ("t_scale", ctypes.c_double),
        ("weight", ctypes.c_double * 4),
        ("tv_weight", ctypes.c_double),
        ("term", CmaxObjective * 4),
    ]


class CmaxBasisObjective(ctypes.Structure):
    """Mirror of cmax_basis_objective_t (include/cmax_hip.h)."""

    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("time_aware", ctypes.c_int32),
        ("T", ctypes.c_int32),
        ("scheme", ctypes.c_int32),
        ("t0", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("basis_dtype", ctypes.c_int32),
        ("scale_later", ctypes.c_int32),  # must be 0
        ("t_scale", ctypes.c_double),
        ("weight", ctypes.c_double * 4),
        ("term", CmaxObjective * 4),
    ]


class CmaxDepthObjective(ctypes.Structure):
    """Mirror of cmax_depth_objective_t (include/cmax_hip.h)."""

    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("time_aware", ctypes.c_int32),
        ("T", ctypes.c_int32),
        ("scheme", ctypes.c_int32),
        ("t0", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("Ka", ctypes.c_int32),
        ("Kb", ctypes.c_int32),
        ("ph", ctypes.c_int32),
        ("pw", ctypes.c_int32),
        ("pad_h", ctypes.c_int32),
        ("pad_w", ctypes.c_int32),
        ("sw_h", ctypes.c_int32),
        ("sw_w", ctypes.c_int32),
        ("basis_dtype", ctypes.c_int32),
        ("scale_later", ctypes.c_int32),  # must be 0
        ("filter_type", ctypes.c_int32),  # must be FILTER_BILINEAR
        ("t_scale", ctypes.c_double),
        ("weight", ctypes.c_double * 4),
        ("tv_weight", ctypes.c_double),  # must be 0
        ("term", CmaxObjective * 4),
    ]


class CmaxDescent(ctypes.Structure):
    """Mirror of cmax_descent_t (include/cmax_hip.h): every value explicit, torch's defaults are filled by `descent_descriptor`."""

    _fields_ = [
        ("method", ctypes.c_int32),
        ("n_iter", ctypes.c_int32),
        ("lr", ctypes.c_double),
        ("lr_step", ctypes.c_int32),
        ("lr_decay", ctypes.c_double),
        ("momentum", ctypes.c_double),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
        ("eps", ctypes.c_double),
    ]


class CmaxDescentResult(ctypes.Structure):
    """Mirror of cmax_descent_result_t (include/cmax_hip.h)."""

    _fields_ = [
        ("best_loss", ctypes.c_double),
        ("best_iter", ctypes.c_int32),
        ("n_done", ctypes.c_int32),
        ("last_lr", ctypes.c_double),
    ]


class CmaxLbfgs(ctypes.Structure):
    """Mirror of cmax_lbfgs_t (include/cmax_hip.h): every value explicit, the defaults are filled by `lbfgs_descriptor`."""

    _fields_ = [
        ("n_eval", ctypes.c_int32),
        ("history", ctypes.c_int32),
        ("max_ls", ctypes.c_int32),
        ("c1", ctypes.c_double),
        ("shrink", ctypes.c_double),
        ("curv_eps", ctypes.c_double),
        ("gtol", ctypes.c_double),
        ("step0", ctypes.c_double),
        ("max_move", ctypes.c_double),
    ]


class CmaxLbfgsResult(ctypes.Structure):
    """Mirror of cmax_lbfgs_result_t (include/cmax_hip.h)."""

    _fields_ = [
        ("final_loss", ctypes.c_double),
        ("gnorm_inf", ctypes.c_double),
        ("last_alpha", ctypes.c_double),
        ("n_iter", ctypes.c_int32),
        ("n_eval_used", ctypes.c_int32),
        ("status", ctypes.c_int32),
    ]


class CmaxFlowRegularizer(ctypes.Structure):
    """Mirror of cmax_flow_regularizer_t (include/cmax_hip.h)."""

    _fields_ = [
        ("kind", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("weight", ctypes.c_double),
        ("eps", ctypes.c_double),
        ("s", ctypes.c_double),
    ]


# constants (include/cmax_hip.h)
F32, F64 = 0, 1
MODEL_2DOF, MODEL_DENSE, MODEL_VOXEL = 0, 1, 2
REF_FIRST, REF_LAST, REF_FRAC = 0, 1, 2
COST_VARIANCE, COST_GRADMAG = 0, 1
COST_MEAN_SQUARE, COST_LAPLACIAN, COST_HESSIAN = 2, 3, 4  # the focus losses (include/cmax_hip.h)
SCHEME_BURGERS, SCHEME_UPWIND = 0, 1
FILTER_BILINEAR, FILTER_NEAREST = 0, 1
OPT_SGD, OPT_ADAM = 0, 1
OPT_CODES = {"SGD": OPT_SGD, "Adam": OPT_ADAM}
DESCENT_MAX_ITER = 4096
DESCENT_MAX_STARTS = 64  # CMAX_DESCENT_MAX_STARTS: trajectories per cmax_objective_descend_batch call
LBFGS_MAX_HISTORY = 16  # CMAX_LBFGS_MAX_HISTORY
LBFGS_STATUS = {0: "BUDGET", 1: "CONVERGED", 2: "LINESEARCH", 3: "BOX", 4: "NONFINITE_START"}  # CMAX_LBFGS_*
LBFGS_CODES = {0: "start", 1: "accepted", 2: "rejected", 3: "reset", 4: "idle"}  # CMAX_LBFGS_CODE_*
LBFGS_FIXED_DOUBLES = 1112  # control block and Gram matrix at the head of the state (csrc/cmax_lbfgs.h)
BASIS_MAX_K = 64  # CMAX_BASIS_MAX_K: fields of a flow basis
BASIS_ADJ_CHUNK = 2048  # CMAX_BASIS_ADJ_CHUNK: elements of [2,H,W] per workgroup of the basis adjoint
DEPTH_ADJ_CHUNK = 1024  # CMAX_DEPTH_ADJ_CHUNK: pixels per workgroup of the depth map's adjoint
FLOWREG_NONE, FLOWREG_DIVERGENCE, FLOWREG_AREA = 0, 1, 2
FLOWREG_CODES = {"divergence": FLOWREG_DIVERGENCE, "area": FLOWREG_AREA}
EINVAL = -1
ABI_VERSION = 4
COMM_ID_BYTES = 128
RAW_LINES = 32
RAW_DOUBLES = RAW_LINES * 16
PROF_CLASSES = 6
ECOMM = -5
EUNSUPPORTED = -6
ENODEV = -4

# every symbol include/cmax_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "cmax_last_error": (ctypes.c_char_p, []),
    "cmax_abi_version": (c_int, []),
    "cmax_tminmax": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp]),
    "cmax_warp_events": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_int, c_int, c_int, c_vp, c_int, c_dbl, c_int,
                                 c_vp, c_vp, c_vp, c_vp]),
    "cmax_warp_events_bwd": (c_int, [c_vp, c_int, c_i64, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_vote": (c_int, [c_vp, c_int, c_i64, c_i64, c_vp, c_dbl, c_int, c_int, c_int, c_int, c_dbl, c_int, c_vp, c_vp]),
    "cmax_vote_bwd": (c_int, [c_vp, c_int, c_i64, c_i64, c_vp, c_dbl, c_int, c_int, c_int, c_int, c_dbl, c_vp, c_vp,
                              c_vp, c_vp]),
    "cmax_blur3": (c_int, [c_vp, c_int, c_int, c_int, c_dbl, c_int, c_vp, c_vp]),
    "cmax_gaussian_filter": (c_int, [c_vp, c_int, c_int, c_int, c_dbl, c_vp, c_vp, c_vp]),
    "cmax_contrast": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "cmax_total_variation": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "cmax_flow_step": (c_int, [c_vp, c_int, c_int, c_int, c_dbl, c_int, c_vp, c_vp]),
    "cmax_set_leaf_deterministic": (c_int, [c_int]),
    "cmax_flow_step_adj": (c_int, [c_vp, c_int, c_int, c_int, c_dbl, c_int, c_vp, c_vp, c_vp]),
    "cmax_voxel_construct": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "cmax_voxel_construct_adj": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "cmax_voxel_construct_tan": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "cmax_voxel_construct_adj_tan": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_patch_to_dense": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "cmax_patch_to_dense_filter": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "cmax_create": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_vp)]),
    "cmax_destroy": (c_int, [c_vp]),
    "cmax_set_events": (c_int, [c_vp, c_vp, c_int, c_i64, c_int, c_dbl, c_dbl, c_int, c_vp]),
    "cmax_set_time_bins": (c_int, [c_vp, c_int, c_vp]),
    "cmax_set_time_slabs": (c_int, [c_vp, c_int, c_vp]),
    "cmax_set_event_weights": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp]),
    "cmax_batch_weighted": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_dbl)]),
    "cmax_set_keep_outside": (c_int, [c_vp, c_int]),
    "cmax_batch_outside": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "cmax_iwe": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_dbl, c_int, c_dbl, c_vp, c_vp]),
    "cmax_objective": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_weight_grad": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "cmax_objective_event_grad": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "cmax_sizeof_iwes": (c_int, []),
    "cmax_iwes": (c_int, [c_vp, ctypes.POINTER(CmaxIwes), c_vp, c_vp, c_vp]),
    "cmax_iwes_vjp": (c_int, [c_vp, ctypes.POINTER(CmaxIwes), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "cmax_iwes_jvp": (c_int, [c_vp, ctypes.POINTER(CmaxIwes), c_vp, c_vp, c_vp, c_vp]),
    "cmax_iwes_vjp_tan": (c_int, [c_vp, ctypes.POINTER(CmaxIwes), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_host": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_has_raw": (c_int, [c_vp, ctypes.POINTER(CmaxObjective)]),
    "cmax_objective_raw": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp]),
    "cmax_finalize_raw_host": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp]),
    "cmax_objective_hvp": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_batch": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_int, c_vp, c_vp, c_vp]),
    "cmax_objective_hvp_dist": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_vote": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, ctypes.POINTER(c_int), c_vp]),
    "cmax_objective_finish": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_int, c_vp, c_vp, c_vp]),
    "cmax_set_deterministic": (c_int, [c_vp, c_int]),
    "cmax_get_deterministic": (c_int, [c_vp, ctypes.POINTER(c_int)]),
    "cmax_comm_available": (c_int, [ctypes.c_char_p, c_int]),
    "cmax_comm_set_c2_bands": (c_int, [c_vp, c_int]),
    "cmax_comm_unique_id": (c_int, [c_vp]),
    "cmax_comm_init": (c_int, [c_vp, c_vp, c_int, c_int]),
    "cmax_comm_destroy": (c_int, [c_vp]),
    "cmax_comm_info": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "cmax_comm_allreduce": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "cmax_objective_dist": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_vp, c_vp, c_vp]),
    "cmax_read_profile_all": (c_int, [c_vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_i64)]),
    "cmax_sizeof_objective": (c_int, []),
    "cmax_set_profiling": (c_int, [c_vp, c_int]),
    "cmax_read_profile": (c_int, [c_vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_i64)]),
    "cmax_copy_iwe": (c_int, [c_vp, c_int, c_vp, c_vp]),
    "cmax_handle_info": (c_int, [c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "cmax_debug_launch_floor": (c_int, [c_vp, c_int, c_vp]),
    "cmax_debug_timeline": (c_int, [c_vp]),
    "cmax_debug_packed_events": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_int), c_vp]),
    "cmax_debug_work_list": (c_int, [c_vp, c_vp, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(c_int), c_vp]),
    "cmax_debug_compact_events": (c_int, [c_vp, c_vp, ctypes.POINTER(c_int), c_vp]),
    "cmax_batch_info": (c_int, [c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "cmax_work_list_info": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "cmax_sizeof_patch_objective": (c_int, []),
    "cmax_patch_plan_create": (c_int, [c_vp, ctypes.POINTER(CmaxPatchObjective), ctypes.POINTER(c_vp)]),
    "cmax_patch_plan_destroy": (c_int, [c_vp]),
    "cmax_patch_plan_info": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "cmax_patch_plan_evaluate": (c_int, [c_vp, c_vp, c_int, ctypes.POINTER(c_dbl), c_vp, c_vp]),
    "cmax_patch_plan_hvp": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_patch_plan_set_t_scale": (c_int, [c_vp, c_dbl]),
    "cmax_sizeof_descent": (c_int, []),
    "cmax_patch_plan_descend": (c_int, [c_vp, c_vp, c_int, ctypes.POINTER(CmaxDescent), ctypes.POINTER(CmaxDescentResult), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_descend": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, ctypes.POINTER(CmaxDescent), ctypes.POINTER(CmaxDescentResult),
                                       c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_descend_batch": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, c_int, ctypes.POINTER(CmaxDescent), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_sizeof_lbfgs": (c_int, []),
    "cmax_patch_plan_lbfgs": (c_int, [c_vp, c_vp, c_int, ctypes.POINTER(CmaxLbfgs), ctypes.POINTER(CmaxLbfgsResult), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_objective_lbfgs": (c_int, [c_vp, ctypes.POINTER(CmaxObjective), c_vp, ctypes.POINTER(CmaxLbfgs), ctypes.POINTER(CmaxLbfgsResult),
                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "cmax_basis_to_dense": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "cmax_sizeof_basis_objective": (c_int, []),
    "cmax_basis_plan_create": (c_int, [c_vp, ctypes.POINTER(CmaxBasisObjective), c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "cmax_depth_to_dense": (c_int, [c_vp] * 5 + [c_int] * 11 + [c_vp, c_vp]),
    "cmax_depth_to_dense_tan": (c_int, [c_vp] * 7 + [c_int] * 11 + [c_vp, c_vp]),
    "cmax_depth_to_dense_adj": (c_int, [c_vp] * 5 + [c_int] * 11 + [c_vp] * 4),
    "cmax_depth_to_dense_adj2": (c_int, [c_vp] * 8 + [c_int] * 11 + [c_vp] * 4),
    "cmax_sizeof_depth_objective": (c_int, []),
    "cmax_depth_plan_create": (c_int, [c_vp, ctypes.POINTER(CmaxDepthObjective), c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "cmax_field_max": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp]),
    "cmax_field_max_adj": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "cmax_sizeof_flow_regularizer": (c_int, []),
    "cmax_flow_regularizer": (c_int, [c_vp, c_int, c_int, c_int, ctypes.POINTER(CmaxFlowRegularizer), c_vp, c_vp, c_vp]),
    "cmax_flow_regularizer_tan": (c_int, [c_vp, c_vp, c_int, c_int, c_int, ctypes.POINTER(CmaxFlowRegularizer), c_vp, c_vp]),
    "cmax_patch_plan_set_flow_regularizer": (c_int, [c_vp, ctypes.POINTER(CmaxFlowRegularizer)]),
    "cmax_patch_search": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_dbl, c_vp, c_vp, c_vp]),
}

_lock = threading.Lock()
_lib = None


def library_path() -> str:
    return _build.LIB_PATH


def load():
    """Load (building in-tree if the .so is missing) and type the library.  Raises on failure."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch first: libcmax_hip.so must bind to the libamdhip64.so.7 torch already loaded so that
        # torch's device pointers and streams are valid inside the library.
        import torch  # noqa: F401

        path = _build.LIB_PATH
        if not os.path.exists(path):
            path = _build.build_library()
        try:
            lib = ctypes.CDLL(path)
        except OSError as e:  # pragma: no cover - environment dependent
            raise RuntimeError(
                f"libcmax_hip.so could not be loaded from {path}: {e}. The HIP extension is the product; "
                "there is no CPU fallback. Build it with `python -m event_based_optical_flow_amd.build`."
            ) from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.cmax_sizeof_objective() != ctypes.sizeof(CmaxObjective):
            raise RuntimeError("cmax_objective_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_iwes() != ctypes.sizeof(CmaxIwes):
            raise RuntimeError("cmax_iwes_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_patch_objective() != ctypes.sizeof(CmaxPatchObjective):
            raise RuntimeError("cmax_patch_objective_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_basis_objective() != ctypes.sizeof(CmaxBasisObjective):
            raise RuntimeError("cmax_basis_objective_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_depth_objective() != ctypes.sizeof(CmaxDepthObjective):
            raise RuntimeError("cmax_depth_objective_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_descent() != ctypes.sizeof(CmaxDescent):
            raise RuntimeError("cmax_descent_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_lbfgs() != ctypes.sizeof(CmaxLbfgs):
            raise RuntimeError("cmax_lbfgs_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_sizeof_flow_regularizer() != ctypes.sizeof(CmaxFlowRegularizer):
            raise RuntimeError("cmax_flow_regularizer_t layout mismatch between libcmax_hip.so and the ctypes binding")
        if lib.cmax_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libcmax_hip ABI {lib.cmax_abi_version()} != binding ABI {ABI_VERSION}")
        _lib = lib
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().cmax_last_error()
        if rc == EUNSUPPORTED:  # a call the library refuses in the handle's state (per-event weights): the library's own text
            raise NotImplementedError(msg.decode("utf-8", "replace") if msg else "unsupported")
        raise CmaxError(rc, msg.decode("utf-8", "replace") if msg else "")


def descent_descriptor(method: str = "Adam", n_iter: int = 100, lr: float = 0.05, lr_step=None, lr_decay: float = 0.1, momentum: float = 0.0,
                       betas=(0.9, 0.999), eps: float = 1e-8) -> CmaxDescent:
    """cmax_descent_t with the reference's constants (src/solver/base.py:857-862: lr 0.05, StepLR(n_iter, 0.1)) and torch's defaults
    for what it leaves to torch.optim (SGD: momentum 0; Adam: betas (0.9, 0.999), eps 1e-8).  lr_step None: n_iter."""
    if method not in OPT_CODES:
        raise NotImplementedError(f"descent method {method!r}: the device-resident loop is built for {sorted(OPT_CODES)}")
    d = CmaxDescent()
    d.method, d.n_iter, d.lr = OPT_CODES[method], int(n_iter), float(lr)
    d.lr_step = int(n_iter if lr_step is None else lr_step)
    d.lr_decay, d.momentum, d.beta1, d.beta2, d.eps = float(lr_decay), float(momentum), float(betas[0]), float(betas[1]), float(eps)
    return d


def flow_regularizer_descriptor(kind, weight: float = 1.0, eps: float = 0.0, s: float = 1.0) -> CmaxFlowRegularizer:
    """cmax_flow_regularizer_t from a kind name ("divergence" | "area") or code; checked here as the library checks it, so that a bad
    parameter is refused without a device: eps >= 0, s > 0, everything finite."""
    import math

    if isinstance(kind, str):
        if kind not in FLOWREG_CODES:
            raise ValueError(f"flow regulariser kind {kind!r}: one of {sorted(FLOWREG_CODES)}")
        code = FLOWREG_CODES[kind]
    else:
        code = int(kind)
        if code not in FLOWREG_CODES.values():
            raise ValueError(f"flow regulariser kind {kind!r}: {FLOWREG_DIVERGENCE} (divergence) or {FLOWREG_AREA} (area)")
    weight, eps, s = float(weight), float(eps), float(s)
    if not (math.isfinite(weight) and math.isfinite(eps) and math.isfinite(s)):
        raise ValueError(f"flow regulariser: weight, eps and s must be finite (got {weight}, {eps}, {s})")
    if eps < 0.0:
        raise ValueError(f"flow regulariser: eps must be >= 0 (got {eps})")
    if s <= 0.0:
        raise ValueError(f"flow regulariser: s must be > 0 (got {s})")
    d = CmaxFlowRegularizer()
    d.kind, d.reserved, d.weight, d.eps, d.s = code, 0, weight, eps, s
    return d


def flow_regularizer_from_config(cfg) -> CmaxFlowRegularizer:
    """... from the dictionary the objectives and the solver key `solver.flow_regularizer` take: {"kind", "weight", "eps", "s"}."""
    if isinstance(cfg, CmaxFlowRegularizer):
        return cfg
    unknown = set(cfg) - {"kind", "weight", "eps", "s"}
    if unknown or "kind" not in cfg:
        raise ValueError(f"flow_regularizer: a dictionary with 'kind' and optionally 'weight', 'eps', 's' (got keys {sorted(cfg)})")
    return flow_regularizer_descriptor(cfg["kind"], cfg.get("weight", 1.0), cfg.get("eps", 0.0), cfg.get("s", 1.0))


class DescentResult:
    """What a device-resident descent returns (cmax_patch_plan_descend / cmax_objective_descend): x_best is the iterate of the lowest
    loss, x_last the iterate after the last step taken (what the reference's run_torch returns as "param": its best_poses aliases the live
    tensor, src/solver/base.py:871); loss_history[it] = L_it (NaN behind a stop); trace [n_iter + 1, nx] or None; n_done steps taken;
    best_iter = -1 and best_loss = inf when no iteration had a finite loss.  `x` and `fun` name x_best / best_loss the way SciPy's result does."""

    def __init__(self, x_best, x_last, best_loss, best_iter, n_done, last_lr, loss_history, trace):
        self.x_best, self.x_last, self.best_loss, self.best_iter = x_best, x_last, float(best_loss), int(best_iter)
        self.n_done, self.last_lr, self.loss_history, self.trace = int(n_done), float(last_lr), loss_history, trace

    @property
    def x(self):
        return self.x_best

    @property
    def fun(self):
        return self.best_loss

    def __repr__(self):
        return f"DescentResult(best_loss={self.best_loss!r}, best_iter={self.best_iter}, n_done={self.n_done}, nx={self.x_best.size})"


def _run_descents(call, K: int, nx: int, descent: CmaxDescent, trace: bool) -> list:
    """Allocates the host outputs of K trajectories, runs `call(descent*, results[K], x_last, x_best, history, trace)` -> K DescentResults
    (views of the [K, ...] host arrays)."""
    import numpy as np

    n_iter = max(int(descent.n_iter), 1)
    res = (CmaxDescentResult * K)()
    x_last, x_best = np.empty((K, nx), dtype=np.float64), np.empty((K, nx), dtype=np.float64)
    hist = np.empty((K, n_iter), dtype=np.float64)
    tr = np.empty((K, n_iter + 1, nx), dtype=np.float64) if trace else None
    check(call(ctypes.byref(descent), res, x_last.ctypes.data, x_best.ctypes.data, hist.ctypes.data, tr.ctypes.data if trace else None))
    return [DescentResult(x_best[z], x_last[z], res[z].best_loss, res[z].best_iter, res[z].n_done, res[z].last_lr, hist[z], tr[z] if trace else None)
            for z in range(K)]


def run_descent(call, nx: int, descent: CmaxDescent, trace: bool) -> DescentResult:
    """The host outputs of a single-start descend entry point (cmax_patch_plan_descend, cmax_objective_descend): one trajectory."""
    return _run_descents(call, 1, nx, descent, trace)[0]


def run_descent_batch(call, K: int, nx: int, descent: CmaxDescent, trace: bool) -> list:
    """... and of the K trajectories of cmax_objective_descend_batch."""
    return _run_descents(call, K, nx, descent, trace)


LBFGS_DEFAULTS = dict(history=8, max_ls=10, c1=1e-4, shrink=0.5, curv_eps=1e-10, gtol=1e-5, step0=1.0, max_move=10.0)


def lbfgs_descriptor(n_eval: int = 32, history: int = 8, max_ls: int = 10, c1: float = 1e-4, shrink: float = 0.5, curv_eps: float = 1e-10,
                     gtol: float = 1e-5, step0: float = 1.0, max_move: float = 10.0) -> CmaxLbfgs:
    """cmax_lbfgs_t (the rules: include/cmax_hip.h).  The library checks the values and names the field it refuses."""
    d = CmaxLbfgs()
    d.n_eval, d.history, d.max_ls = int(n_eval), int(history), int(max_ls)
    d.c1, d.shrink, d.curv_eps, d.gtol, d.step0, d.max_move = float(c1), float(shrink), float(curv_eps), float(gtol), float(step0), float(max_move)
    return d


def lbfgs_state_bytes(nx: int, history: int, n_eval: int, trace: bool) -> int:
    """The size of the L-BFGS state as include/cmax_hip.h documents it (a 2-DoF handle holds 16 doubles more in front of it)."""
    return 8 * (LBFGS_FIXED_DOUBLES + (4 + 2 * history) * nx + 2 * n_eval + (n_eval + 1) // 2 + ((n_eval + 1) * nx if trace else 0))


class LbfgsResult:
    """What a device-resident L-BFGS solve returns (cmax_patch_plan_lbfgs / cmax_objective_lbfgs), named the way SciPy's result is: x
    the accepted point, fun its loss, status a word of LBFGS_STATUS (status_code the number), nit accepted steps, nfev evaluations up to
    the terminating one, success = CONVERGED; loss_history / alpha / code [n_eval] per evaluation (codes: LBFGS_CODES), trace
    [n_eval + 1, nx] or None, gnorm_inf, last_alpha."""

    def __init__(self, x, res, loss_history, alpha, code, trace):
        self.x, self.fun, self.gnorm_inf, self.last_alpha = x, float(res.final_loss), float(res.gnorm_inf), float(res.last_alpha)
        self.status_code, self.status = int(res.status), LBFGS_STATUS[int(res.status)]
        self.nit, self.nfev, self.success = int(res.n_iter), int(res.n_eval_used), int(res.status) == 1
        self.loss_history, self.alpha, self.code, self.trace = loss_history, alpha, code, trace

    @property
    def accepted_losses(self):
        """The losses of the accepted points in order (start included): non-increasing by construction."""
        return self.loss_history[(self.code == 0) | (self.code == 1)]

    def __repr__(self):
        return f"LbfgsResult(fun={self.fun!r}, status={self.status!r}, nit={self.nit}, nfev={self.nfev}, nx={self.x.size})"


def run_lbfgs(call, nx: int, lbfgs: CmaxLbfgs, trace: bool) -> LbfgsResult:
    """Allocates the host outputs, runs `call(lbfgs*, result*, x, loss_history, alpha, code, trace)` -> LbfgsResult."""
    import numpy as np

    n = max(int(lbfgs.n_eval), 1)
    res, x = CmaxLbfgsResult(), np.empty(nx, dtype=np.float64)
    hist, alpha, code = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int32)
    tr = np.empty((n + 1, nx), dtype=np.float64) if trace else None
    check(call(ctypes.byref(lbfgs), ctypes.byref(res), x.ctypes.data, hist.ctypes.data, alpha.ctypes.data, code.ctypes.data, tr.ctypes.data if trace else None))
    return LbfgsResult(x, res, hist, alpha, code, tr)


def require_gpu():
    """The product path needs a real device; never degrade silently."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "event_based_optical_flow_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False and "
            "there is no CPU fallback for the contrast-maximization kernels."
        )
