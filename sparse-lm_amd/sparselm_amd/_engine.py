"""ctypes binding of the C ABI in ``include/slm_engine.h`` (``libslm_hip.so``).

This is the only place Python touches the HIP engine.  There is no CPU fallback: if the shared
library is missing, or no gfx950 device is visible, every entry point raises.  The GIL is released
for the duration of each foreign call (ctypes does that for ``CDLL`` functions).

The boundary mirrors ``CVXRegressor._solve(X, y, solver_options) -> beta`` of the reference
(src/sparselm/model/_base.py:512-519): ``Dataset`` holds the preprocessed ``(X, y)`` in HBM and
``Dataset.solve_path`` returns the minimiser(s).
"""

from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import weakref

import numpy as np

_LIB_NAME = "libslm_hip.so"
_LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")

SLM_OK = 0
SLM_ERR_BAD_ARG = 1
SLM_ERR_OOM = 2
SLM_ERR_HIP = 3
SLM_ERR_NO_DEVICE = 4
SLM_ERR_COMM = 5
SLM_ERR_NOT_CONVERGED = 6
SLM_ERR_NON_FINITE = 7
SLM_ERR_UNSUPPORTED = 8

FLAG_NO_RESTART = 1
FLAG_PROFILE = 2
FLAG_COLD_START = 4
FLAG_FRESH_L = 8
FLAG_FISTA_ONLY = 16
FLAG_WORKING_SET = 32  # force the Gram-assisted refinement even for small X
FLAG_NO_WORKING_SET = 64
FLAG_ON_CHIP = 128  # problems whose Gram matrix fits a workgroup: one launch per call (csrc/small_kernels.hpp)
FLAG_COVARIANCE = 256  # passes from the Grams of the call's row sets (Dataset.covariance; csrc/cov_kernels.hpp)
FLAG_PROFILE_UNIT = 1024  # with FLAG_PROFILE: the event bracket spans residuals + X^T R, the whole gradient unit of the split pass
FLAG_NO_MODEL_GRAM = 512  # lanes beyond the working set's 512 columns take plain steps, no rounds on the model Gram (csrc/mg_kernels.hpp)

COMM_ID_BYTES = 128
ABI_VERSION = 24  # SLM_ABI_VERSION of include/slm_engine.h this binding was written against
L0_GRID_MAX = 128  # SLM_L0_GRID_MAX: the problems of one slm_solve_l0_profile_grid call
L0_LOCAL_PMAX = 1024  # SLM_L0_LOCAL_PMAX: the columns of slm_solve_l0_local
L0_LOCAL_MAX_PROBLEMS = 8192  # SLM_L0_LOCAL_MAX_PROBLEMS: the (cell, start) problems of one slm_solve_l0_local call

# every symbol include/slm_engine.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "slm_abi_version",
    "slm_last_error",
    "slm_device_count",
    "slm_host_alloc",
    "slm_host_free",
    "slm_engine_create",
    "slm_engine_destroy",
    "slm_engine_synchronize",
    "slm_reload_knobs",
    "slm_engine_device_info",
    "slm_dataset_create",
    "slm_dataset_create_device",
    "slm_dataset_create_synthetic",
    "slm_dataset_nonfinite",
    "slm_dataset_destroy",
    "slm_dataset_shape",
    "slm_dataset_download",
    "slm_dataset_center",
    "slm_dataset_set_row_weights",
    "slm_dataset_set_targets",
    "slm_dataset_clone",
    "slm_dataset_set_groups",
    "slm_dataset_lipschitz",
    "slm_dataset_max_lanes",
    "slm_dataset_path_lanes",
    "slm_gradient",
    "slm_gradient_ex",
    "slm_gradient_lanes",
    "slm_working_set_lanes",
    "slm_working_set_model_solve",
    "slm_eval_sse",
    "slm_eval_sse_sparse",
    "slm_dense_spd_solve",
    "slm_solve_path",
    "slm_solve_lanes",
    "slm_solve_lanes_reweighted",
    "slm_solve_path_lanes",
    "slm_solve_standardized_sgl",
    "slm_solve_constrained",
    "slm_solve_l0",
    "slm_solve_l0_l1",
    "slm_solve_l0_profile",
    "slm_solve_l0_wide",
    "slm_solve_l0_profile_wide",
    "slm_solve_l0_profile_batch",
    "slm_solve_l0_profile_grid",
    "slm_solve_l0_l1_profile",
    "slm_solve_l0_l1_profile_wide",
    "slm_solve_l0_constrained",
    "slm_solve_l0_xb",
    "slm_solve_l0_xb_wide",
    "slm_solve_l0_local",
    "slm_solve_l0_local_descent",
    "slm_solve_l0_local_folds",
    "slm_solve_l0_local_subsets",
    "slm_solve_l0_local_groups",
    "slm_solve_l0_local_l1",
    "slm_solve_l0_local_bound",
    "slm_solve_l0_local_nodes",
    "slm_solve_l0_local_prove",
    "slm_solve_l0_local_group_nodes",
    "slm_solve_l0_local_group_prove",
    "slm_dataset_covariance",
    "slm_dataset_covariance_folds",
    "slm_dataset_covariance_folds_begin",
    "slm_dataset_covariance_folds_finish",
    "slm_dataset_covariance_count",
    "slm_dataset_covariance_clear",
    "slm_dataset_covariance_download",
    "slm_dataset_model_gram",
    "slm_dataset_read_ceiling",
    "slm_dataset_set_replicated",
    "slm_comm_unique_id",
    "slm_comm_init",
    "slm_comm_info",
    "slm_comm_collectives",
    "slm_comm_all_reduce_probe",
    "slm_comm_init_local",
    "slm_dataset_set_global_rows",
    "slm_comm_destroy",
)


class EngineError(RuntimeError):
    """HIP / RCCL / device failure reported by the engine."""


class NonFiniteError(EngineError):
    """The iterate became non-finite (counterpart of cvxpy's SolverError / 'infeasible')."""


class _PenaltyStruct(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("d", C.c_void_p)]


class _GradientOpts(C.Structure):
    _fields_ = [("route", C.c_int32), ("n_lanes", C.c_int32), ("lane_out", C.c_int32), ("probe_lanes", C.c_int32),
                ("xtr_only", C.c_int32)]


WSL_GATHER_X = 1  # slm_working_set_lanes: gather from the row-major X, not the column-major copy
WSL_XTY = 2       # ... and queue the ws_xty kernels with every build
WSL_XTY_BUILD = 4  # ... X_W^T y with every build the way a solve gets it (out of the gather where it reads the column-major copy)


class _WsLanesOpts(C.Structure):
    _fields_ = [("route", C.c_int32), ("n_lanes", C.c_int32), ("Z", C.c_void_p), ("on_ws", C.c_void_p),
                ("row_weights", C.c_void_p), ("n_eff", C.c_void_p), ("cov_index", C.c_void_p), ("cols", C.c_void_p),
                ("k_end", C.c_void_p), ("n_builds", C.c_int32), ("flags", C.c_uint32)]


# slm_working_set_model_solve flags
WMS_DIRECT, WMS_HARD, WMS_INVALID, WMS_BUILDING, WMS_DISABLED, WMS_STALE, WMS_NONFINITE = 1, 2, 4, 8, 16, 32, 64
WMS_COUNTERS = ("refined", "inner_iters", "newton_steps", "newton_fails", "newton_nopd", "newton_factors", "newton_unknowns",
                "hard_next")


class _WsModelOpts(C.Structure):
    _fields_ = [("n_lanes", C.c_int32), ("kreal", C.c_int32), ("cols", C.c_void_p), ("n_sets", C.c_int32), ("flags", C.c_uint32),
                ("gram", C.c_void_p), ("set_of", C.c_void_p), ("zprev", C.c_void_p), ("gprev", C.c_void_p), ("z", C.c_void_p),
                ("a0", C.c_void_p), ("b0", C.c_void_p), ("d0", C.c_void_p), ("points", C.c_void_p), ("tol", C.c_void_p),
                ("mode", C.c_void_p), ("Lw", C.c_void_p), ("repeats", C.c_void_p), ("last_point", C.c_void_p),
                ("last_cols", C.c_void_p)]


class _WsModelOut(C.Structure):
    _fields_ = [("z", C.c_void_p), ("beta", C.c_void_p), ("served", C.c_void_p), ("mu", C.c_void_p), ("zsup", C.c_void_p),
                ("t", C.c_void_p), ("have_base", C.c_void_p), ("zzero", C.c_void_p), ("want_full", C.c_void_p),
                ("repeats", C.c_void_p), ("hard_lane", C.c_void_p), ("last_point", C.c_void_p), ("Lw", C.c_void_p),
                ("counters", C.c_void_p), ("kernels", C.c_void_p), ("kernels_len", C.c_int32)]


class _PathPoint(C.Structure):
    _fields_ = [("sa", C.c_double), ("sb", C.c_double), ("sd", C.c_double), ("extrap", C.c_double)]


class _SolveOpts(C.Structure):
    _fields_ = [
        ("tol", C.c_double),
        ("max_iter", C.c_int32),
        ("check_every", C.c_int32),
        ("L", C.c_double),
        ("flags", C.c_uint32),
    ]


class _PointInfo(C.Structure):
    _fields_ = [
        ("n_iter", C.c_int32),
        ("status", C.c_int32),
        ("resid", C.c_double),
        ("beta_norm", C.c_double),
        ("loss", C.c_double),
        ("L", C.c_double),
        ("mode", C.c_int32),
        ("rejects", C.c_int32),
        ("kkt", C.c_double),
        ("mu", C.c_double),
    ]


class _SolveStats(C.Structure):
    _fields_ = [
        ("grad_launches", C.c_int64),
        ("grad_timed", C.c_int64),
        ("grad_ms_total", C.c_double),
        ("wall_ms", C.c_double),
        ("lipschitz_ms", C.c_double),
        ("ws_builds", C.c_int64),
        ("ws_appends", C.c_int64),
        ("ws_refined", C.c_int64),
        ("ws_misses", C.c_int64),
        ("ws_columns", C.c_int64),
        ("ws_inner_iters", C.c_int64),
        ("ws_direct_steps", C.c_int64),
        ("mg_rounds", C.c_int64),
        ("mg_inner_iters", C.c_int64),
        ("mg_rejected", C.c_int64),
        ("mg_build_ms", C.c_double),
        ("light_passes", C.c_int64),
        ("light_columns", C.c_int64),
    ]


class _Lane(C.Structure):
    _fields_ = [
        ("pen", C.POINTER(_PenaltyStruct)),
        ("points", C.POINTER(_PathPoint)),
        ("n_points", C.c_int32),
        ("beta0", C.c_void_p),
        ("row_weight", C.c_void_p),
        ("n_eff", C.c_int64),
        ("betas_out", C.c_void_p),
        ("group_norms_out", C.c_void_p),
        ("infos", C.POINTER(_PointInfo)),
    ]


class _Reweight(C.Structure):
    _fields_ = [
        ("coef_scale", C.c_double),
        ("group_scale", C.c_void_p),
        ("numerator", C.c_double),
        ("eps", C.c_double),
        ("tol", C.c_double),
        ("n_coef", C.c_int32),
        ("n_group", C.c_int32),
    ]


MAX_LANES = 16  # lanes of a call of independent problems (a half of the split pass: the sixteen columns of an MFMA operand)
MAX_LANES_WIDE = 32  # SLM_MAX_LANES: lanes a shared path may run on -- two halves on one read of X (xtr32_mfma_kernel)
MAX_CELLS = 64  # SLM_MAX_CELLS: lanes of a call the on-chip solver takes (Dataset.max_lanes tells which limit applies)

# numpy views of the two per-point structs (no per-point Python objects on the way in or out)
_INFO_DTYPE = np.dtype(
    [("n_iter", "<i4"), ("status", "<i4"), ("resid", "<f8"), ("beta_norm", "<f8"), ("loss", "<f8"), ("L", "<f8"),
     ("mode", "<i4"), ("rejects", "<i4"), ("kkt", "<f8"), ("mu", "<f8")]
)
assert _INFO_DTYPE.itemsize == C.sizeof(_PointInfo) and C.sizeof(_PathPoint) == 32


def _points_block(pts, gam):
    """(K, 4) float64 rows (sa, sb, sd, extrap) == slm_path_point[K]"""
    out = np.empty((pts.shape[0], 4))
    out[:, :3] = pts
    out[:, 3] = gam
    return out


def _as(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))

WS_COLUMNS = 512  # WS_KCAP of the engine: columns a working set / a sparse scoring call can hold

_lib = None
_lib_lock = threading.Lock()


def library_path() -> str:
    return os.environ.get("SLM_HIP_LIBRARY", os.path.join(_LIB_DIR, _LIB_NAME))


def load_library():
    """dlopen the engine; raises ``EngineError`` with build instructions if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise EngineError(
                f"{path} not found: build the HIP engine first "
                "(python -c 'import __graft_entry__ as g; g.build()' or "
                "`python sparse-lm_amd/build.py`). sparselm_amd has no CPU fallback."
            )
        try:
            lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError as exc:  # missing ROCm runtime etc.
            raise EngineError(f"cannot load {path}: {exc}") from exc
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        P = C.POINTER
        lib.slm_abi_version.restype = C.c_int
        lib.slm_last_error.restype = C.c_char_p
        if lib.slm_abi_version() != ABI_VERSION:
            raise EngineError(
                f"{path} has ABI version {lib.slm_abi_version()}, this binding needs {ABI_VERSION}: "
                "rebuild it with `python sparse-lm_amd/build.py --force`"
            )
        sigs = {
            "slm_device_count": [P(C.c_int)],
            "slm_engine_create": [C.c_int, P(vp)],
            "slm_engine_destroy": [vp],
            "slm_engine_synchronize": [vp],
            "slm_engine_device_info": [vp, P(i64), C.c_char_p, C.c_int],
            "slm_dataset_create": [vp, vp, i64, i64, i64, i64, vp, vp, P(vp)],
            "slm_dataset_create_device": [vp, vp, i64, i64, i64, vp, vp, P(vp)],
            "slm_dataset_create_synthetic": [vp, i64, i64, C.c_uint64, i64, vp, dbl, P(vp)],
            "slm_dataset_nonfinite": [vp, P(i32)],
            "slm_host_alloc": [C.c_size_t, P(vp)],
            "slm_host_free": [vp],
            "slm_dataset_destroy": [vp],
            "slm_dataset_shape": [vp, P(i64), P(i64), P(i64)],
            "slm_dataset_download": [vp, vp, vp],
            "slm_dataset_center": [vp, vp, P(dbl)],
            "slm_dataset_set_row_weights": [vp, vp],
            "slm_dataset_set_targets": [vp, vp],
            "slm_dataset_clone": [vp, vp, P(vp)],
            "slm_dataset_set_groups": [vp, vp, i32],
            "slm_dataset_lipschitz": [vp, P(dbl)],
            "slm_dataset_max_lanes": [vp, C.c_uint32, P(i32)],
            "slm_dataset_path_lanes": [vp, i32, C.c_uint32, P(i32)],
            "slm_gradient": [vp, vp, vp, P(dbl), i32, P(dbl)],
            "slm_gradient_ex": [vp, vp, P(_GradientOpts), vp, P(dbl), i32, P(dbl)],
            "slm_gradient_lanes": [vp, i32, i32, vp, vp, vp, vp, i64, vp, vp, C.c_char_p, i32],
            "slm_working_set_lanes": [vp, P(_WsLanesOpts), vp, vp, vp, vp, vp, vp, vp, C.c_char_p, i32],
            "slm_working_set_model_solve": [vp, P(_WsModelOpts), P(_WsModelOut)],
            "slm_reload_knobs": [],
            "slm_eval_sse": [vp, vp, i32, vp, vp],
            "slm_eval_sse_sparse": [vp, vp, i32, vp, i32, vp, vp],
            "slm_dense_spd_solve": [vp, vp, i32, vp, vp, P(dbl)],
            "slm_solve_path": [
                vp,
                P(_PenaltyStruct),
                P(_PathPoint),
                i32,
                P(_SolveOpts),
                vp,
                vp,
                vp,
                P(_PointInfo),
                P(_SolveStats),
            ],
            "slm_solve_lanes": [vp, P(_Lane), i32, P(_SolveOpts), P(_SolveStats)],
            "slm_solve_lanes_reweighted": [vp, P(_Lane), P(_Reweight), i32, P(_SolveOpts), P(_SolveStats), P(i32)],
            "slm_solve_path_lanes": [
                vp, P(_PenaltyStruct), P(_PathPoint), i32, i32, P(_SolveOpts), vp, vp, vp, P(_PointInfo), P(_SolveStats),
            ],
            "slm_solve_standardized_sgl": [vp, vp, vp, P(_SolveOpts), dbl, i32, vp, i32, vp, vp, P(_PointInfo)],
            "slm_solve_constrained": [vp, vp, vp, i32, vp, vp, P(_SolveOpts), dbl, i32, vp, i32, vp, vp, P(_PointInfo)],
            "slm_solve_l0": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, P(C.c_uint64), P(dbl), P(i64), P(_PointInfo)],
            "slm_solve_l0_l1": [vp, dbl, dbl, dbl, vp, i64, vp, P(C.c_uint64), P(dbl), P(i64), P(_PointInfo)],
            "slm_solve_l0_profile": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, vp, vp, P(i64), P(_PointInfo)],
            "slm_solve_l0_wide": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, vp, P(dbl), P(i64), P(_PointInfo)],
            "slm_solve_l0_profile_wide": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, vp, vp, P(i64), P(_PointInfo)],
            "slm_solve_l0_l1_profile": [vp, dbl, i32, dbl, dbl, vp, i64, vp, vp, vp, P(i64), P(_PointInfo)],
            "slm_solve_l0_l1_profile_wide": [vp, dbl, i32, dbl, dbl, vp, i64, vp, vp, vp, P(i64), P(_PointInfo)],
            "slm_solve_l0_profile_batch": [vp, i32, vp, vp, i32, dbl, i32, dbl, vp, dbl, vp, i64, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_profile_grid": [vp, i32, vp, vp, i32, i32, vp, i32, dbl, i32, vp, dbl, vp, i64, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_xb": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, P(C.c_uint64), P(dbl), P(i64), P(_PointInfo)],
            "slm_solve_l0_xb_wide": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, vp, P(dbl), P(i64), P(_PointInfo)],
            "slm_solve_l0_constrained": [vp, dbl, i32, dbl, vp, dbl, vp, i64, vp, i32, vp, vp, vp, vp, i32, vp, P(C.c_uint64), P(dbl), P(i64),
                                         vp, P(_PointInfo)],
            "slm_solve_l0_local": [vp, i32, vp, vp, dbl, i32, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_descent": [vp, i32, vp, vp, dbl, i32, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_folds": [vp, i32, vp, vp, i32, i32, vp, vp, dbl, i32, vp, i32, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_subsets": [vp, i32, vp, vp, i32, i32, vp, vp, dbl, i32, vp, i32, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_groups": [vp, i32, vp, vp, i32, i32, vp, vp, dbl, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_l1": [vp, i32, vp, vp, i32, i32, vp, vp, vp, dbl, i32, vp, i32, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_bound": [vp, i32, vp, vp, dbl, vp, i32, dbl, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_nodes": [vp, i32, vp, vp, dbl, i32, vp, vp, vp, vp, vp, i32, dbl, vp, vp, vp, vp, vp, P(_PointInfo)],
            "slm_solve_l0_local_prove": [vp, i32, vp, vp, dbl, vp, dbl, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                         P(_PointInfo)],
            "slm_solve_l0_local_group_nodes": [vp, i32, vp, vp, dbl, i32, vp, vp, vp, vp, vp, vp, vp, i32, dbl, vp, vp, vp, vp, vp,
                                               P(_PointInfo)],
            "slm_solve_l0_local_group_prove": [vp, i32, vp, vp, dbl, vp, vp, vp, dbl, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                               vp, vp, vp, vp, P(_PointInfo)],
            "slm_dataset_covariance": [vp, vp, i64],
            "slm_dataset_covariance_folds": [vp, vp, vp, i32],
            "slm_dataset_covariance_folds_begin": [vp, vp, vp, i32, P(i32)],
            "slm_dataset_covariance_folds_finish": [vp],
            "slm_dataset_covariance_count": [vp, P(i32)],
            "slm_dataset_covariance_clear": [vp],
            "slm_dataset_covariance_download": [vp, i32, vp, vp, vp],
            "slm_dataset_model_gram": [vp, vp],
            "slm_dataset_read_ceiling": [vp, i32, P(dbl), P(dbl)],
            "slm_dataset_set_replicated": [vp, i32],
            "slm_comm_unique_id": [vp],
            "slm_comm_init": [vp, i32, i32, vp],
            "slm_comm_info": [vp, P(i32), P(i32)],
            "slm_comm_collectives": [vp, P(i64)],
            "slm_comm_all_reduce_probe": [vp, i64, i32, P(dbl)],
            "slm_comm_init_local": [P(vp), i32, dbl],
            "slm_dataset_set_global_rows": [vp, i64],
            "slm_comm_destroy": [vp],
        }
        for name, argtypes in sigs.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        _lib = lib
        return lib


_binding = None  # the compiled binding of the hot calls (csrc/binding.cpp), False when it is not to be used


def load_binding():
    """The pybind11 module over the hot calls (``slm_solve_lanes``, ``slm_solve_path_lanes``, ``slm_dataset_create``), or
    None: built next to the engine by ``sparse-lm_amd/build.py``; ``SLM_NO_BINDING=1`` (A/B runs, the ABI tests) and a library
    taken from ``SLM_HIP_LIBRARY`` (the module is linked against the one in ``_lib``) leave every call to ctypes."""
    global _binding
    if _binding is None:
        lib = load_library()
        # (SLM_BINDING_PATH: another build of the same module -- tools/sanitize.sh loads the ASan + UBSan one)
        path = os.environ.get("SLM_BINDING_PATH") or os.path.join(_LIB_DIR, "_slm_binding.so")
        if os.environ.get("SLM_NO_BINDING") or os.environ.get("SLM_HIP_LIBRARY") or not os.path.exists(path):
            _binding = False
        else:
            import importlib.util

            spec = importlib.util.spec_from_file_location("_slm_binding", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            if mod.abi_version() != lib.slm_abi_version() or mod.info_record_bytes() != _INFO_DTYPE.itemsize:
                # a module left over from another ABI: an accelerator that does not fit is not used (ctypes serves every
                # call), and says so once
                import warnings

                warnings.warn(f"{path} does not match libslm_hip.so (rebuild with `python sparse-lm_amd/build.py --force`): "
                              "falling back on the ctypes binding", RuntimeWarning)
                _binding = False
            else:
                mod.set_error_types(EngineError, NonFiniteError)
                _binding = mod
    return _binding or None


def _check(rc: int):
    if rc == SLM_OK:
        return
    msg = (_lib.slm_last_error() or b"").decode("utf-8", "replace")
    if rc == SLM_ERR_BAD_ARG:
        raise ValueError(msg)
    if rc == SLM_ERR_OOM:
        raise MemoryError(msg)
    if rc == SLM_ERR_NON_FINITE:
        raise NonFiniteError(msg)
    if rc == SLM_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise EngineError(f"[slm status {rc}] {msg}")


def device_count() -> int:
    lib = load_library()
    n = C.c_int(0)
    rc = lib.slm_device_count(C.byref(n))
    return n.value if rc == SLM_OK else 0


def _f64(arr, name, shape=None):
    a = np.ascontiguousarray(arr, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name} has shape {a.shape}, expected {shape}")
    return a


def _ptr(a):
    # (the address as an int: what a c_void_p argument or field takes; `ctypes.data_as` costs twice as much, and a
    #  sixteen-lane call asks eighty times)
    return None if a is None else a.ctypes.data


_extrap_cache: dict = {}  # bytes of the points -> secant factors (the folds and rows of a grid walk the same path)


def path_extrapolation(pts) -> np.ndarray:
    """Secant factors gamma_k = (s_k - s_{k-1}) / (s_{k-1} - s_{k-2}) for a path whose points are all
    multiples s_k of one penalty direction (rank-one (K, 3) array); zeros otherwise."""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    key = pts.tobytes()
    hit = _extrap_cache.get(key)
    if hit is None:
        hit = _path_extrapolation(pts)
        if len(_extrap_cache) >= 4096:  # (a grid cut into pieces brings a few hundred distinct ones)
            _extrap_cache.clear()
        _extrap_cache[key] = hit
    return hit.copy()


def _path_extrapolation(pts) -> np.ndarray:
    K = pts.shape[0]
    gam = np.zeros(K)
    if K < 3:
        return gam
    ref = pts[np.argmax(np.abs(pts).sum(axis=1))]
    nrm = float(ref @ ref)
    if nrm <= 0.0:
        return gam
    s = pts @ ref / nrm
    # (plain array arithmetic: this runs between two solves, with the device idle -- a Python loop over the points
    #  and np.allclose cost 0.15 ms per 50-point path, 3 % of the solve itself)
    if np.max(np.abs(s[:, None] * ref[None, :] - pts)) > 1e-12 * np.max(np.abs(pts)):
        return gam  # the penalty changes shape along the path: prediction would be meaningless
    den = s[1:-1] - s[:-2]
    num = s[2:] - s[1:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = num / den
    ok = (den != 0.0) & np.isfinite(g) & (np.abs(g) <= 10.0)
    gam[2:] = np.where(ok, g, 0.0)
    return gam


def lane_points(segments) -> tuple[np.ndarray, np.ndarray]:
    """(points, extrap) of a lane that walks several pieces of paths one after the other (the lanes
    ``distributed.plan_lane_calls`` plans): ``segments`` is a list of (K_s, 3) arrays in the order the lane takes
    them; the secant factors are those of each piece on its own, zero on the first two points of every piece (the
    two solutions before them belong to another path)."""
    pts = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1, 3) for s in segments]
    return np.vstack(pts), np.concatenate([path_extrapolation(s) for s in pts])


_STATS_FIELDS = ("grad_launches", "grad_timed", "grad_ms_total", "wall_ms", "lipschitz_ms", "ws_builds", "ws_appends",
                 "ws_refined", "ws_misses", "ws_columns", "ws_inner_iters", "ws_direct_steps", "mg_rounds", "mg_inner_iters",
                 "mg_rejected", "mg_build_ms", "light_passes", "light_columns")


class PathResult:
    """The solutions of one lane's path.  ``betas`` (n_points, p) and ``group_norms`` (n_points, G) or None are views of the
    call's result blocks; the per-point records and the call's statistics are read where they are asked for (a
    sixteen-lane call used to build 160 small arrays nobody looked at):

    ``n_iter``, ``status`` (SLM_OK or SLM_ERR_NOT_CONVERGED), ``resid``, ``beta_norm``, ``loss``, ``mode`` (1 = spectral
    steps, 0 = FISTA, 2 = the on-chip solver), ``kkt`` (KKT residual at exit), ``mu`` (strong-convexity estimate the point
    was accepted with), ``L_points`` (inverse step of the step that produced the point): arrays of n_points; ``L``: inverse
    step at the last point; ``converged``; and the statistics of the
    call, shared by its lanes: ``grad_launches``, ``grad_timed``, ``grad_ms_total``, ``wall_ms``, ``lipschitz_ms``,
    ``ws_builds`` (working sets selected from scratch; 0: refinement not used), ``ws_appends``, ``ws_refined``,
    ``ws_misses``, ``ws_columns`` (columns in the working set at the end), ``ws_inner_iters``, ``ws_direct_steps``,
    ``mg_rounds`` / ``mg_inner_iters`` / ``mg_rejected`` / ``mg_build_ms`` (the model Gram: rounds of lanes beyond the
    working set, their inner iterations, proposals the true objective rejected, build time inside the call),
    ``light_passes`` / ``light_columns`` (re-verifications after a miss that were certified partial passes instead of passes
    over X -- csrc/light_kernels.hpp -- and the borderline columns they read; not counted in ``grad_launches``)."""

    __slots__ = ("betas", "group_norms", "_infos", "_stats")

    def __init__(self, betas, group_norms, infos, stats):
        self.betas, self.group_norms, self._infos, self._stats = betas, group_norms, infos, stats

    n_iter = property(lambda self: self._infos["n_iter"].astype(np.int64))
    status = property(lambda self: self._infos["status"].astype(np.int64))
    resid = property(lambda self: self._infos["resid"].copy())
    beta_norm = property(lambda self: self._infos["beta_norm"].copy())
    loss = property(lambda self: self._infos["loss"].copy())
    mode = property(lambda self: self._infos["mode"].astype(np.int64))
    kkt = property(lambda self: self._infos["kkt"].copy())
    mu = property(lambda self: self._infos["mu"].copy())
    L = property(lambda self: float(self._infos["L"][-1]))
    L_points = property(lambda self: self._infos["L"].copy())  # inverse step of every point at exit (1 / s of its last step)

    @property
    def converged(self) -> bool:
        return not self._infos["status"].any()  # (SLM_OK == 0)

    def __getattr__(self, name):  # the call's statistics
        try:
            v = self._stats[_STATS_FIELDS.index(name)]
        except ValueError:
            raise AttributeError(name) from None
        return float(v) if name in ("grad_ms_total", "wall_ms", "lipschitz_ms", "mg_build_ms") else int(v)


def _stats_tuple(stats) -> tuple:
    return tuple(getattr(stats, f) for f in _STATS_FIELDS)


def _path_result(betas, gn, infos, K, stats) -> PathResult:
    return PathResult(betas, gn, infos, stats if isinstance(stats, tuple) else _stats_tuple(stats))


_live_engines: "weakref.WeakSet[Engine]" = weakref.WeakSet()


class Engine:
    """An engine owns a HIP stream and, optionally, an RCCL communicator.  ``get_engine`` hands out one per
    (process, device); further ones on the same device (``Engine(device_id)``) are further streams: solves on
    different engines run side by side -- the launches between the passes of one beside the passes of the other."""

    def __init__(self, device_id: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.slm_engine_create(int(device_id), C.byref(h)))
        self._h = h
        self.device_id = int(device_id)
        self._datasets = weakref.WeakSet()  # closed before the engine goes (their handles point at it)
        self._pid = os.getpid()
        _live_engines.add(self)  # (every engine, not only the per-device defaults, is released in order at exit)

    def close(self):
        if getattr(self, "_h", None):
            for ds in list(getattr(self, "_datasets", ())):
                ds.close()
            self._lib.slm_engine_destroy(self._h)
            self._h = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self._lib.slm_engine_synchronize(self._h))

    def device_info(self) -> dict:
        out = (C.c_int64 * 6)()
        name = C.create_string_buffer(256)
        _check(self._lib.slm_engine_device_info(self._h, out, name, 256))
        return {
            "name": name.value.decode(),
            "compute_units": out[0],
            "lds_bytes_per_cu": out[1],
            "hbm_total_bytes": out[2],
            "hbm_free_bytes": out[3],
            "wavefront": out[4],
            "clock_khz": out[5],
        }

    # -- datasets -----------------------------------------------------------------------------
    def dataset(self, X, y, row_weight=None) -> "Dataset":
        _sync_knobs()
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be 2-D")
        if not (X.flags.c_contiguous or X.flags.f_contiguous):
            X = np.ascontiguousarray(X)
        n, p = X.shape
        y = _f64(y, "y", (n,))
        rw = None if row_weight is None else _f64(row_weight, "row_weight", (n,))
        rs, cs = (X.strides[0] // 8, X.strides[1] // 8)
        if X.flags.c_contiguous:
            rs, cs = p, 1
        elif X.flags.f_contiguous:
            rs, cs = 1, n
        b = load_binding()
        if b is not None:
            return Dataset(self, C.c_void_p(b.dataset_create(self._h.value, X, y, rw)), n, p)
        h = C.c_void_p()
        _check(self._lib.slm_dataset_create(self._h, _ptr(X), n, p, rs, cs, _ptr(y), _ptr(rw), C.byref(h)))
        return Dataset(self, h, n, p)

    def dataset_from_device(self, dX_ptr: int, n: int, p: int, ld: int, dy_ptr: int, drw_ptr: int = 0):
        _sync_knobs()
        h = C.c_void_p()
        _check(
            self._lib.slm_dataset_create_device(
                self._h, C.c_void_p(dX_ptr), n, p, ld, C.c_void_p(dy_ptr), C.c_void_p(drw_ptr or None), C.byref(h)
            )
        )
        return Dataset(self, h, n, p)

    def synthetic_dataset(self, n, p, seed, coef, noise_sd=0.0, row_offset=0) -> "Dataset":
        _sync_knobs()
        coef = _f64(coef, "coef", (p,))
        h = C.c_void_p()
        _check(
            self._lib.slm_dataset_create_synthetic(
                self._h, n, p, C.c_uint64(seed), row_offset, _ptr(coef), float(noise_sd), C.byref(h)
            )
        )
        return Dataset(self, h, n, p)

    # -- row-sharded mode -----------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(self._lib.slm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank: int, n_ranks: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._lib.slm_comm_init(self._h, rank, n_ranks, buf))

    def comm_destroy(self):
        _check(self._lib.slm_comm_destroy(self._h))

    def comm_info(self) -> tuple[int, int]:
        """(rank, ranks) of the communicator as RCCL reports them; (0, 1) without one."""
        r, n = C.c_int32(), C.c_int32()
        _check(self._lib.slm_comm_info(self._h, C.byref(r), C.byref(n)))
        return int(r.value), int(n.value)

    def comm_ranks(self) -> int:
        return self.comm_info()[1]

    def comm_collectives(self) -> int:
        """All-reduces this engine has entered since its communicator was created."""
        n = C.c_int64()
        _check(self._lib.slm_comm_collectives(self._h, C.byref(n)))
        return int(n.value)

    def comm_all_reduce_us(self, count: int, reps: int = 20) -> float:
        """Microseconds per all-reduce of ``count`` doubles on this engine's communicator (every rank calls it alike)."""
        us = C.c_double()
        _check(self._lib.slm_comm_all_reduce_probe(self._h, int(count), int(reps), C.byref(us)))
        return float(us.value)

    # -- diagnostics ------------------------------------------------------------------------------
    def dense_spd_solve(self, H, rhs):
        """(H^-1 rhs, lambda_min estimate) by the model solver's one-workgroup Cholesky (m <= 512)."""
        H = _f64(H, "H")
        m = H.shape[0]
        if H.shape != (m, m):
            raise ValueError("H must be square")
        rhs = _f64(rhs, "rhs", (m,))
        x = np.empty(m)
        mu = C.c_double()
        _check(self._lib.slm_dense_spd_solve(self._h, _ptr(H), m, _ptr(rhs), _ptr(x), C.byref(mu)))
        return x, mu.value


class Dataset:
    """Device-resident (X, y[, row weights][, groups]) plus the solver state that goes with it."""

    def __init__(self, engine: Engine, handle, n: int, p: int):
        self.engine = engine
        self._lib = engine._lib
        self._h = handle
        self.n, self.p = int(n), int(p)
        self.n_groups = self.p
        engine._datasets.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.slm_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def ld(self) -> int:
        n, p, ld = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib.slm_dataset_shape(self._h, C.byref(n), C.byref(p), C.byref(ld)))
        return ld.value

    def download(self, want_X=True, want_y=True):
        X = np.empty((self.n, self.p)) if want_X else None
        y = np.empty(self.n) if want_y else None
        _check(self._lib.slm_dataset_download(self._h, _ptr(X), _ptr(y)))
        return X, y

    def nonfinite(self) -> int:
        """``slm_dataset_nonfinite``: 0 when the uploaded X is finite throughout, bit 0 for a NaN, bit 1 for an infinity."""
        kind = C.c_int32()
        _check(self._lib.slm_dataset_nonfinite(self._h, C.byref(kind)))
        return int(kind.value)

    def center(self):
        """Centre the device copy of (X, y) in place by the row-weighted means; returns (x_mean, y_mean)."""
        _sync_knobs()
        xm = np.empty(self.p)
        ym = C.c_double()
        _check(self._lib.slm_dataset_center(self._h, _ptr(xm), C.byref(ym)))
        return xm, ym.value

    def set_row_weights(self, row_weight):
        rw = None if row_weight is None else _f64(row_weight, "row_weight", (self.n,))
        _check(self._lib.slm_dataset_set_row_weights(self._h, _ptr(rw)))

    def clone(self, engine: "Engine | None" = None) -> "Dataset":
        """A copy of this dataset (X, y, row weights; device to device) on ``engine`` -- default: a new engine
        on the same device, i.e. a further stream.  Group structure is set again by the caller."""
        eng = Engine(self.engine.device_id) if engine is None else engine
        h = C.c_void_p()
        _check(self._lib.slm_dataset_clone(self._h, eng._h, C.byref(h)))
        return Dataset(eng, h, self.n, self.p)

    def set_targets(self, y):
        """Replace y on the device (X and what was derived from it stay)."""
        yv = _f64(y, "y", (self.n,))
        _check(self._lib.slm_dataset_set_targets(self._h, _ptr(yv)))

    def set_global_rows(self, n_global: int):
        _check(self._lib.slm_dataset_set_global_rows(self._h, int(n_global)))

    def set_groups(self, gidx, n_groups=None):
        """``gidx``: dense group index per feature (0..G-1, reference order model/_lasso.py:248)."""
        if gidx is None:
            _check(self._lib.slm_dataset_set_groups(self._h, None, 0))
            self.n_groups = self.p
            return
        g = np.ascontiguousarray(gidx, dtype=np.int32)
        if g.shape != (self.p,):
            raise ValueError(f"gidx must have shape ({self.p},)")
        G = int(g.max()) + 1 if n_groups is None else int(n_groups)
        _check(self._lib.slm_dataset_set_groups(self._h, _ptr(g), G))
        self.n_groups = G

    def max_lanes(self, flags: int = 0) -> int:
        """Lanes one ``solve_lanes`` call can take here (16 in working-set solves on large X, else what the
        fused kernel table has for this p)."""
        _sync_knobs()
        out = C.c_int32()
        _check(self._lib.slm_dataset_max_lanes(self._h, int(flags), C.byref(out)))
        return int(out.value)

    def path_lanes(self, n_points: int, flags: int = 0) -> int:
        """The lane count ``solve_path(..., lanes=0)`` runs a path of ``n_points`` on (``slm_dataset_path_lanes``)."""
        _sync_knobs()
        out = C.c_int32()
        _check(self._lib.slm_dataset_path_lanes(self._h, int(n_points), int(flags), C.byref(out)))
        return int(out.value)

    def lipschitz(self) -> float:
        _sync_knobs()
        L = C.c_double()
        _check(self._lib.slm_dataset_lipschitz(self._h, C.byref(L)))
        return L.value

    def gradient(self, z=None, reps: int = 0, split: bool = False, lanes: int = 1, lane: int = 0, probe_lanes: int = 1,
                 xtr_only: bool = False):
        """g = X^T W (X z - y)/n, loss = 1/(2n)||Xz - y||_W^2[, mean kernel ms over ``reps`` launches].

        ``split=True``: by the split pass (residuals from X, then X^T R for all lane slots on one read) with ``lanes`` lanes
        all standing at z, the gradient of lane ``lane`` returned -- how the parity tests reach xtr18 / xtr20 / xtr32 and the
        rowdot kernels through the boundary (slm_gradient_ex); ``probe_lanes`` / ``xtr_only``: the timed launches."""
        _sync_knobs()
        zz = None if z is None else _f64(z, "z", (self.p,))
        g = np.empty(self.p)
        loss = C.c_double()
        ms = C.c_double()
        if not split and lanes == 1 and probe_lanes == 1:
            _check(self._lib.slm_gradient(self._h, _ptr(zz), _ptr(g), C.byref(loss), int(reps), C.byref(ms) if reps > 0 else None))
        else:
            o = _GradientOpts(1 if split else 0, int(lanes), int(lane), int(probe_lanes), 1 if xtr_only else 0)
            _check(self._lib.slm_gradient_ex(self._h, _ptr(zz), C.byref(o), _ptr(g), C.byref(loss), int(reps),
                                             C.byref(ms) if reps > 0 else None))
        return (g, loss.value, ms.value) if reps > 0 else (g, loss.value)

    def sample_product(self):
        """``slm_gradient_ex`` route 2: what a cold shared path opens on -- ``g = -X_s^T y / n_s`` and the loss at zero over the
        first ``n // SLM_SAMPLE_DIV`` rows, through the dataset's fp32 image of those rows where it has one (the fp64 rows with
        ``SLM_SAMPLE_F64=1`` or where a float cannot hold X).  Returns ``(g, loss)``."""
        _sync_knobs()
        g = np.empty(self.p)
        loss = C.c_double()
        o = _GradientOpts(2, 1, 0, 1, 0)
        _check(self._lib.slm_gradient_ex(self._h, None, C.byref(o), _ptr(g), C.byref(loss), 0, None))
        return g, loss.value

    def gradient_lanes(self, Z, row_weights=None, n_eff=None, route: int = 0, cov_index=None, n_rows: int = 0):
        """``slm_gradient_lanes``: one gradient pass of ``len(Z)`` lanes through route 0 (fused), 1 (split pass) or 2
        (covariance entries ``cov_index``), each lane with its own point ``Z[l]``, row weights ``row_weights[l]`` and
        ``n_eff[l]``; ``n_rows`` > 0: only the first rows.  Returns ``(G, loss, kernels)``: (lanes, p), (lanes,) and the
        names of the kernels launched.  A route without a kernel for the call raises NotImplementedError.  On a row-sharded
        dataset (routes 0 and 1, every rank calling alike): ``row_weights`` are this rank's rows, ``n_eff`` is the job's, and
        every rank gets the all-reduced gradients and losses."""
        _sync_knobs()
        Z = _f64(np.atleast_2d(Z), "Z")
        B = Z.shape[0]
        if Z.shape[1] != self.p:
            raise ValueError(f"Z must have {self.p} columns")
        rw = None if row_weights is None else _f64(row_weights, "row_weights", (B, self.n))
        ne = None if n_eff is None else _f64(n_eff, "n_eff", (B,))
        ci = None if cov_index is None else np.ascontiguousarray(cov_index, dtype=np.int32)
        if ci is not None and ci.shape != (B,):
            raise ValueError(f"cov_index has shape {ci.shape}, expected {(B,)}")
        G = np.empty((B, self.p))
        loss = np.empty(B)
        names = C.create_string_buffer(512)
        _check(self._lib.slm_gradient_lanes(self._h, int(route), B, _ptr(Z), _ptr(rw), _ptr(ne), _ptr(ci), int(n_rows),
                                            _ptr(G), _ptr(loss), names, len(names)))
        return G, loss, names.value.decode()

    def working_set_lanes(self, Z, cols, k_end, on_ws=None, row_weights=None, n_eff=None, route: int = 1, cov_index=None,
                          gather_from_x: bool = False, xty: bool = False, want_xw: bool = False, xty_build: bool = False):
        """``slm_working_set_lanes``: W built in stages -- ``cols[:k_end[0]]``, then each ``cols[k_end[b-1]:k_end[b]]``
        appended -- and one gradient pass of ``len(Z)`` lanes on it through route 1 (split pass; residuals from W for the
        lanes with ``on_ws``) or 2 (covariance entries ``cov_index``).  Returns a namespace: ``G`` (lanes, p), ``loss``,
        ``gram`` (row sets, K, K), ``set_of``, ``n_sets``, ``K``, ``XW`` (n, K) with ``want_xw``, ``xty`` (-X_W^T y / n) and
        ``yy`` (y^T y / 2n) with ``xty`` (the two ws_xty kernels behind the gather) or ``xty_build`` (the way a solve
        gets them on this dataset: out of the gather), and ``kernels``.  A call no kernel serves raises NotImplementedError.
        On a row-sharded dataset (route 1, no ``xty``, every rank calling alike): ``row_weights`` and ``XW`` are this rank's
        rows, ``n_eff`` is the job's, ``gram`` / ``G`` / ``loss`` are over all rows and ``set_of`` is agreed among the ranks."""
        import types

        _sync_knobs()
        Z = _f64(np.atleast_2d(Z), "Z")
        B = Z.shape[0]
        if Z.shape[1] != self.p:
            raise ValueError(f"Z must have {self.p} columns")
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        k_end = np.ascontiguousarray(np.atleast_1d(k_end), dtype=np.int32)
        if k_end.size == 0 or cols.size < int(k_end[-1]):
            raise ValueError("cols must hold k_end[-1] feature indices")
        kreal = int(k_end[-1])
        K = max(16, (kreal + 15) // 16 * 16)
        ow = None if on_ws is None else np.ascontiguousarray(np.broadcast_to(np.asarray(on_ws, dtype=np.int32), (B,)))
        rw = None if row_weights is None else _f64(row_weights, "row_weights", (B, self.n))
        ne = None if n_eff is None else _f64(n_eff, "n_eff", (B,))
        ci = None if cov_index is None else np.ascontiguousarray(cov_index, dtype=np.int32)
        if ci is not None and ci.shape != (B,):
            raise ValueError(f"cov_index has shape {ci.shape}, expected {(B,)}")
        opts = _WsLanesOpts(int(route), B, _ptr(Z), _ptr(ow), _ptr(rw), _ptr(ne), _ptr(ci), _ptr(cols), _ptr(k_end),
                            int(k_end.size), (WSL_GATHER_X if gather_from_x else 0) | (WSL_XTY if xty else 0) |
                            (WSL_XTY_BUILD if xty_build else 0))
        G = np.empty((B, self.p))
        loss = np.empty(B)
        set_of = np.empty(B, dtype=np.int32)
        n_sets = C.c_int32(0)
        gram = np.empty((B, K, K))
        XW = np.empty((self.n, K)) if want_xw else None
        xt = np.empty(kreal + 2) if (xty or xty_build) else None
        names = C.create_string_buffer(4096)
        _check(self._lib.slm_working_set_lanes(self._h, C.byref(opts), _ptr(G), _ptr(loss), _ptr(set_of), C.byref(n_sets),
                                               _ptr(gram), _ptr(XW), _ptr(xt), names, len(names)))
        ns = n_sets.value
        return types.SimpleNamespace(G=G, loss=loss, gram=gram[:ns], set_of=set_of, n_sets=ns, K=K, XW=XW,
                                     xty=None if xt is None else xt[:kreal], yy=None if xt is None else float(xt[kreal]),
                                     touched_outside=int(xt[kreal + 1]) if xty_build else None, kernels=names.value.decode())

    def ws_build(self, cols, k_end=None, xty: bool = False, gather_from_x: bool = False, want_xw: bool = False):
        """The builds of a working set alone, as a solve queues them: ``working_set_lanes`` with one lane at zero.  ``xty``:
        the exact linear term of the build behind a row-sample pass (``xty`` = -X_W^T y / n per position, ``yy`` = y^T y / 2n),
        with the kernels a solve takes for it on this dataset; ``touched_outside`` counts the entries of the gradient vector
        outside W that the builds wrote to (a pad position must write nothing: 0)."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        r = self.working_set_lanes(np.zeros((1, self.p)), cols, [cols.size] if k_end is None else k_end, on_ws=[0],
                                   gather_from_x=gather_from_x, want_xw=want_xw, xty_build=xty)
        return r

    def working_set_model_solve(self, cols, gram, zprev, gprev, z, a0, b0, d0, points, tol, mode, set_of=None, Lw=None,
                                direct: bool = True, hard: bool = False, invalid: bool = False, building: bool = False,
                                disabled: bool = False, stale: bool = False, allow_nonfinite: bool = False, repeats=None,
                                last_point=None, last_cols=None, flags: int = 0):
        """``slm_working_set_model_solve``: the working-set model solver alone, one launch (two with ``direct``) over
        ``len(z)`` lanes, on the model ``gprev_W . (x - zprev)_W + (x - zprev)_W^T gram (x - zprev)_W / 2 + pen(x)`` with W =
        ``cols``.  ``gram`` is (sets, K, K) with K = max(16, len(cols) rounded up to 16), zero on the padding.  Per lane:
        ``zprev``, ``gprev``, ``z``, ``a0`` (lanes, p), ``b0``, ``d0`` (lanes, G), ``points`` (lanes, 3), ``tol``, ``mode``.
        Returns a namespace with ``z``, ``beta`` (NaN where nothing was written), the per-lane ``served``, ``mu``, ``zsup``,
        ``t``, ``have_base``, ``zzero`` (presets -1, -1, 7, 1, 1), ``want_full``, ``repeats``, ``hard_lane``, ``last_point``,
        ``Lw`` per Gram, the ``WMS_COUNTERS`` by name, and ``kernels``."""
        import types

        _sync_knobs()
        z = _f64(np.atleast_2d(z), "z")
        B = z.shape[0]
        if z.shape[1] != self.p:
            raise ValueError(f"z must have {self.p} columns")
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        kreal = int(cols.size)
        K = max(16, (kreal + 15) // 16 * 16)
        gram = _f64(gram, "gram")
        if gram.ndim == 2:
            gram = gram[None]
        if gram.ndim != 3 or gram.shape[1:] != (K, K):
            raise ValueError(f"gram has shape {gram.shape}, expected (sets, {K}, {K})")
        gram = np.ascontiguousarray(gram)
        ns = gram.shape[0]
        zprev = _f64(zprev, "zprev", (B, self.p))
        gprev = _f64(gprev, "gprev", (B, self.p))
        a0 = _f64(a0, "a0", (B, self.p))
        b0 = _f64(np.atleast_2d(b0), "b0")
        d0 = _f64(np.atleast_2d(d0), "d0")
        if b0.shape != d0.shape or b0.shape[0] != B:
            raise ValueError("b0 and d0 must have shape (lanes, groups)")
        points = _f64(points, "points", (B, 3))
        tol = _f64(np.broadcast_to(np.asarray(tol, dtype=np.float64), (B,)), "tol", (B,))

        def ints(v, count):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (count,)))

        mode = ints(mode, B)
        so, rp, lp, lc = ints(set_of, B), ints(repeats, B), ints(last_point, B), ints(last_cols, B)
        lw = None if Lw is None else _f64(np.broadcast_to(np.asarray(Lw, dtype=np.float64), (ns,)), "Lw", (ns,))
        fl = int(flags) | (WMS_DIRECT if direct else 0) | (WMS_HARD if hard else 0) | (WMS_INVALID if invalid else 0) | \
            (WMS_BUILDING if building else 0) | (WMS_DISABLED if disabled else 0) | (WMS_STALE if stale else 0) | \
            (WMS_NONFINITE if allow_nonfinite else 0)
        opts = _WsModelOpts(B, kreal, _ptr(cols), ns, fl, _ptr(gram), _ptr(so), _ptr(zprev), _ptr(gprev), _ptr(z), _ptr(a0),
                            _ptr(b0), _ptr(d0), _ptr(points), _ptr(tol), _ptr(mode), _ptr(lw), _ptr(rp), _ptr(lp), _ptr(lc))
        o = types.SimpleNamespace(z=np.empty((B, self.p)), beta=np.empty((B, self.p)))
        for name in ("served", "zsup", "have_base", "zzero", "want_full", "repeats", "hard_lane", "last_point"):
            setattr(o, name, np.zeros(B, dtype=np.int32))
        o.mu, o.t, o.Lw = np.zeros(B), np.zeros(B), np.zeros(ns)
        counters = np.zeros(8, dtype=np.int32)
        names = C.create_string_buffer(256)
        out = _WsModelOut(_ptr(o.z), _ptr(o.beta), _ptr(o.served), _ptr(o.mu), _ptr(o.zsup), _ptr(o.t), _ptr(o.have_base),
                          _ptr(o.zzero), _ptr(o.want_full), _ptr(o.repeats), _ptr(o.hard_lane), _ptr(o.last_point), _ptr(o.Lw),
                          _ptr(counters), C.cast(names, C.c_void_p), len(names))
        _check(self._lib.slm_working_set_model_solve(self._h, C.byref(opts), C.byref(out)))
        for name, v in zip(WMS_COUNTERS, counters):
            setattr(o, name, int(v))
        o.K = K
        o.kernels = names.value.decode()
        return o

    def eval_sse(self, Z, row_weight=None, sparse=None) -> np.ndarray:
        """sum_i w_i (x_i . Z[k] - y_i)^2 for every row Z[k] of ``Z`` (m, p); ``row_weight`` is e.g. the
        test mask of a CV fold.  Rows with a joint support of at most 512 columns are scored from those
        columns (``sparse=False`` forces the dense route: ceil(m/4) passes over the resident X)."""
        _sync_knobs()
        Z = _f64(np.atleast_2d(Z), "Z")
        if Z.shape[1] != self.p:
            raise ValueError(f"Z must have {self.p} columns")
        rw = None if row_weight is None else _f64(row_weight, "row_weight", (self.n,))
        out = np.empty(Z.shape[0])
        # sparse rows (the solutions of a path): gather the union of their supports once on the device
        # and score from those columns instead of passes over X
        cols = np.flatnonzero(np.any(Z != 0.0, axis=0)).astype(np.int32)
        if cols.size == 0:
            cols = np.zeros(1, dtype=np.int32)
        if cols.size <= WS_COLUMNS and sparse is not False:
            Zs = np.ascontiguousarray(Z[:, cols])
            _check(self._lib.slm_eval_sse_sparse(self._h, _ptr(cols), int(cols.size), _ptr(Zs), Z.shape[0], _ptr(rw),
                                                 _ptr(out)))
            return out
        _check(self._lib.slm_eval_sse(self._h, _ptr(Z), Z.shape[0], _ptr(rw), _ptr(out)))
        return out

    def solve_lanes(
        self,
        lanes,
        tol: float = 1e-8,
        max_iter: int = 10000,
        check_every: int = 0,
        L: float = 0.0,
        flags: int = 0,
        want_group_norms: bool = False,
        extrapolate: bool = True,
        _reweighted: bool = False,
    ) -> list:
        """Solve up to MAX_LANES independent warm-started paths on ONE pass over X per iteration.

        ``lanes``: list of dicts with ``points`` (K_l, 3) and optionally ``a``, ``b``, ``d``,
        ``beta0``, ``row_weight`` (length n, e.g. a CV-fold mask), ``n_eff`` (1/n scaling, e.g. the
        number of training rows) and ``extrap`` (K_l secant factors, see ``lane_points``; default: derived from
        the points).  Returns one ``PathResult`` per lane (shared timing fields).
        """
        _sync_knobs()
        nl = len(lanes)
        if not (1 <= nl <= MAX_CELLS):
            raise ValueError(f"between 1 and {MAX_CELLS} lanes, got {nl}")
        G = self.n_groups
        b = load_binding()
        if b is not None:  # the compiled binding marshals the lanes itself
            rounds = None
            if _reweighted:
                betas, gnb, inf, ks, st, rounds = b.solve_lanes_reweighted(
                    self._h.value, list(lanes), self.n, self.p, G, float(tol), int(max_iter), int(check_every), float(L),
                    int(flags), bool(want_group_norms), _host_pool.empty)
            else:
                betas, gnb, inf, ks, st = b.solve_lanes(self._h.value, list(lanes), self.n, self.p, G, float(tol), int(max_iter),
                                                        int(check_every), float(L), int(flags), bool(want_group_norms),
                                                        bool(extrapolate), _host_pool.empty)
            infos, out, at, p = inf.view(_INFO_DTYPE), [], 0, self.p
            for K in ks:
                out.append(PathResult(betas[at * p : (at + K) * p].reshape(K, p),
                                      gnb[at * G : (at + K) * G].reshape(K, G) if want_group_norms else None, infos[at : at + K], st))
                at += K
            return (out, [int(r) for r in rounds]) if _reweighted else out
        keep = []  # keep every buffer alive for the duration of the call
        clanes = (_Lane * nl)()
        outs = []
        # one block for the coefficients of all lanes (and one for their group norms): the engine fetches buffers
        # that follow each other in one copy
        k_all = [int(np.asarray(spec["points"]).size // 3) for spec in lanes]
        beta_block = _host_pool.empty(sum(k_all) * self.p)
        gn_block = _host_pool.empty(sum(k_all) * G) if want_group_norms else None
        infos_block = np.zeros(sum(k_all), dtype=_INFO_DTYPE)  # (one block: buffers that follow each other travel together)
        at = 0
        for l, spec in enumerate(lanes):
            pts = np.ascontiguousarray(spec["points"], dtype=np.float64).reshape(-1, 3)
            K = pts.shape[0]
            if spec.get("extrap") is not None:  # (lanes that walk pieces of several paths bring their own factors)
                gam = _f64(spec["extrap"], "extrap", (K,))
            else:
                gam = path_extrapolation(pts) if extrapolate else np.zeros(K)
            cpts = _points_block(pts, gam)

            def vec(name, size):
                v = spec.get(name)
                if v is None:
                    return None
                v = np.asarray(v)
                return _f64(v if v.shape == (size,) else np.broadcast_to(v, (size,)), name)

            a_, b_, d_ = vec("a", self.p), vec("b", G), vec("d", G)
            pen = _PenaltyStruct(_ptr(a_), _ptr(b_), _ptr(d_))
            b0 = None if spec.get("beta0") is None else _f64(spec["beta0"], "beta0", (self.p,))
            rw = None if spec.get("row_weight") is None else _f64(spec["row_weight"], "row_weight", (self.n,))
            betas = beta_block[at * self.p : (at + K) * self.p].reshape(K, self.p)
            gn = gn_block[at * G : (at + K) * G].reshape(K, G) if want_group_norms else None
            infos = infos_block[at : at + K]
            at += K
            keep.append((cpts, a_, b_, d_, pen, b0, rw))
            clanes[l].pen = C.pointer(pen)
            clanes[l].points = _as(cpts, _PathPoint)
            clanes[l].n_points = K
            clanes[l].beta0 = _ptr(b0)
            clanes[l].row_weight = _ptr(rw)
            clanes[l].n_eff = int(spec.get("n_eff") or 0)
            clanes[l].betas_out = _ptr(betas)
            clanes[l].group_norms_out = _ptr(gn)
            clanes[l].infos = _as(infos, _PointInfo)
            outs.append((betas, gn, infos, K))
        opts = _SolveOpts(float(tol), int(max_iter), int(check_every), float(L), int(flags))
        stats = _SolveStats()
        if _reweighted:
            rules, rounds = (_Reweight * nl)(), (C.c_int32 * nl)()
            for l, spec in enumerate(lanes):
                coef_scale, group_scale, numerator, eps, rtol, n_coef, n_group = spec["reweight"]
                gsc = None if group_scale is None else _f64(np.broadcast_to(np.asarray(group_scale), (int(n_group),)), "group_scale")
                keep.append(gsc)
                rules[l] = _Reweight(float(coef_scale), _ptr(gsc), float(numerator), float(eps), float(rtol), int(n_coef), int(n_group))
            _check(self._lib.slm_solve_lanes_reweighted(self._h, clanes, rules, nl, C.byref(opts), C.byref(stats), rounds))
            return [_path_result(betas, gn, infos, K, stats) for betas, gn, infos, K in outs], [int(r) for r in rounds]
        _check(self._lib.slm_solve_lanes(self._h, clanes, nl, C.byref(opts), C.byref(stats)))
        return [_path_result(betas, gn, infos, K, stats) for betas, gn, infos, K in outs]

    def solve_lanes_reweighted(self, lanes, tol: float = 1e-8, max_iter: int = 10000, flags: int = 0, want_group_norms: bool = True):
        """The re-weighting loops of Adaptive* estimators inside one launch (``slm_solve_lanes_reweighted``): every lane dict
        has ``points`` = its rounds (``max_iter`` rows, normally all ones) and ``reweight`` = ``(coef_scale, group_scale or
        None, numerator, eps, tol, n_coef, n_group)``.  Returns ``(results, rounds)``: one ``PathResult`` per lane with a row
        per round, and the number of rounds each lane ran (its last solution is row ``rounds - 1``).
        ``NotImplementedError`` when the problem is not one the on-chip solver takes, or a round did not settle there: the
        caller then loops over ``solve_lanes`` itself."""
        return self.solve_lanes(lanes, tol=tol, max_iter=max_iter, flags=int(flags) | FLAG_ON_CHIP, want_group_norms=want_group_norms,
                                extrapolate=False, _reweighted=True)

    def solve_path(
        self,
        points,
        a=None,
        b=None,
        d=None,
        beta0=None,
        tol: float = 1e-8,
        max_iter: int = 10000,
        check_every: int = 0,
        L: float = 0.0,
        flags: int = 0,
        want_group_norms: bool = False,
        extrapolate: bool = True,
        lanes: int = 1,
    ) -> PathResult:
        """Warm-started path; ``points`` is (K, 3) of (sa, sb, sd) scales applied to (a, b, d).

        ``a`` (p,), ``b`` (G,), ``d`` (G,): ``None`` means all ones.  K == 1 is the reference's
        single ``_solve``.  ``extrapolate``: when all points are multiples of one penalty direction
        (an alpha path), start point k from the secant prediction through the two previous solutions.
        ``lanes`` > 1 cuts the path into that many contiguous sub-paths that advance together, one
        pass over X serving all of them (the first point of every later sub-path starts cold).
        ``lanes=0``: the engine's choice (``slm_solve_path_lanes`` with ``n_lanes = 0``: sixteen, or eighteen / twenty
        where that saves a pass over a large X).
        """
        _sync_knobs()
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        K = pts.shape[0]
        lanes = 0 if int(lanes) == 0 and K > 1 else max(1, min(int(lanes), MAX_LANES_WIDE, K))  # (the engine takes as many as the dataset's kernels serve)
        common = dict(a=a, b=b, d=d)
        kw = dict(tol=tol, max_iter=max_iter, check_every=check_every, L=L, flags=flags,
                  want_group_norms=want_group_norms, extrapolate=extrapolate)
        if lanes == 1:
            return self.solve_lanes([dict(points=pts, beta0=beta0, **common)], **kw)[0]
        # shared path: the engine splits it into `lanes` ranges and balances them by work stealing
        G = self.n_groups
        bnd = load_binding()
        if bnd is not None:
            betas, gnb, inf, st = bnd.solve_path_lanes(self._h.value, pts, self.p, G, a, b, d, beta0, int(lanes), float(tol),
                                                       int(max_iter), int(check_every), float(L), int(flags),
                                                       bool(want_group_norms), bool(extrapolate), _host_pool.empty)
            return PathResult(betas.reshape(K, self.p), gnb.reshape(K, G) if want_group_norms else None, inf.view(_INFO_DTYPE), st)
        gam = path_extrapolation(pts) if extrapolate else np.zeros(K)
        cpts = _points_block(pts, gam)
        a_ = None if a is None else _f64(np.broadcast_to(a, (self.p,)), "a")
        b_ = None if b is None else _f64(np.broadcast_to(b, (G,)), "b")
        d_ = None if d is None else _f64(np.broadcast_to(d, (G,)), "d")
        pen = _PenaltyStruct(_ptr(a_), _ptr(b_), _ptr(d_))
        b0 = None if beta0 is None else _f64(beta0, "beta0", (self.p,))
        opts = _SolveOpts(float(tol), int(max_iter), int(check_every), float(L), int(flags))
        betas = _host_pool.empty(K * self.p).reshape(K, self.p)
        gn = _host_pool.empty(K * G).reshape(K, G) if want_group_norms else None
        infos = np.zeros(K, dtype=_INFO_DTYPE)
        stats = _SolveStats()
        _check(
            self._lib.slm_solve_path_lanes(
                self._h, C.byref(pen), _as(cpts, _PathPoint), K, lanes, C.byref(opts), _ptr(b0), _ptr(betas), _ptr(gn),
                _as(infos, _PointInfo), C.byref(stats),
            )
        )
        return _path_result(betas, gn, infos, K, stats)


    def covariance(self, row_weight=None, n_eff=0):
        """``slm_dataset_covariance``: build (or find) the Gram of the row set ``(row_weight, n_eff)`` -- what a lane
        brings as ``row_weight`` / ``n_eff`` -- so that solves with ``FLAG_COVARIANCE`` take their gradients from it
        instead of reading X.  Worth it when many solves share the row set (a fold of a large grid)."""
        _sync_knobs()
        rw = None if row_weight is None else _f64(row_weight, "row_weight", (self.n,))
        _check(self._lib.slm_dataset_covariance(self._h, _ptr(rw), int(n_eff)))

    def covariance_folds(self, row_weights, n_effs):
        """``slm_dataset_covariance_folds``: the Grams of the training sets of a K-fold split at once -- where the test rows
        partition the rows, the Gram of all rows is the sum of the test rows' Grams and is never formed from X."""
        _sync_knobs()
        rws = [_f64(w, "row_weight", (self.n,)) for w in row_weights]
        if not 1 <= len(rws) <= MAX_LANES:
            raise ValueError(f"between 1 and {MAX_LANES} row sets")
        ptrs = (C.c_void_p * len(rws))(*[w.ctypes.data for w in rws])
        ne = (C.c_int64 * len(rws))(*[int(v) for v in n_effs])
        _check(self._lib.slm_dataset_covariance_folds(self._h, ptrs, ne, len(rws)))

    def covariance_folds_begin(self, row_weights, n_effs) -> bool:
        """First half of ``covariance_folds``: queues the products of THIS rank's rows (all rows without a communicator)
        and returns; False when the masks are no K-fold partition (nothing queued: use ``covariance``)."""
        _sync_knobs()
        rws = [_f64(w, "row_weight", (self.n,)) for w in row_weights]
        if not 1 <= len(rws) <= MAX_LANES:
            raise ValueError(f"between 1 and {MAX_LANES} row sets")
        ptrs = (C.c_void_p * len(rws))(*[w.ctypes.data for w in rws])
        ne = (C.c_int64 * len(rws))(*[int(v) for v in n_effs])
        started = C.c_int32()
        _check(self._lib.slm_dataset_covariance_folds_begin(self._h, ptrs, ne, len(rws), C.byref(started)))
        return bool(started.value)

    def covariance_folds_finish(self):
        """Second half: a replica among ranks sums the parts over the ranks here (the grid mode's one collective), then the
        folds' Grams are formed and filed."""
        _check(self._lib.slm_dataset_covariance_folds_finish(self._h))

    def covariance_download(self, index: int):
        """(G, c, {yy, n_eff, fp}) of Gram ``index`` (oldest first): diagnostics and tests."""
        G = np.empty((self.p, self.p))
        c = np.empty(self.p)
        sc = np.empty(4)
        _check(self._lib.slm_dataset_covariance_download(self._h, int(index), _ptr(G), _ptr(c), _ptr(sc)))
        return G, c, {"yy": float(sc[0]), "n_eff": float(sc[1]), "fingerprint": (float(sc[2]), float(sc[3]))}

    def read_ceiling(self, reps: int = 5) -> tuple[float, float]:
        """(GB/s, ms per sweep) of a read-only stream over the device copy of X: plain 16-byte loads, summed up -- the ceiling
        the passes over X are read against on this device."""
        _sync_knobs()
        gbs, ms = C.c_double(), C.c_double()
        _check(self._lib.slm_dataset_read_ceiling(self._h, int(reps), C.byref(gbs), C.byref(ms)))
        return float(gbs.value), float(ms.value)

    def model_gram(self, download: bool = False):
        """Build the model Gram of the dataset now (``csrc/mg_kernels.hpp``: ``X^T W X / n`` from an fp16 product, what lanes
        beyond the working set's 512 columns iterate on between two passes over X; solves build it themselves when they
        need it).  ``download=True`` returns it as an (ld, ld) array (tests)."""
        _sync_knobs()
        ld = (self.p + 15) // 16 * 16
        G = np.empty((ld, ld)) if download else None
        _check(self._lib.slm_dataset_model_gram(self._h, _ptr(G) if download else None))
        return G

    def set_replicated(self, replicated: bool = True):
        """On an engine with a communicator: this dataset holds ALL rows (grid mode), not a row block -- no per-pass
        collective; the communicator only carries the folds' Grams (``covariance_folds``)."""
        _check(self._lib.slm_dataset_set_replicated(self._h, int(bool(replicated))))

    def covariance_clear(self):
        """Drop every Gram built so far (later solves run over X)."""
        _check(self._lib.slm_dataset_covariance_clear(self._h))

    def covariance_count(self) -> int:
        out = C.c_int32()
        _check(self._lib.slm_dataset_covariance_count(self._h, C.byref(out)))
        return int(out.value)

    def solve_standardized_sgl(self, a, b, beta0=None, warm=False, tol=1e-8, tol_inner=0.0, max_sweeps=0,
                               max_iter=0, want_group_norms=False):
        """``slm_solve_standardized_sgl``: the splitting for ``l1 + sum_g b_g ||X_g beta_g||_2`` with all sweeps in
        one launch.  Returns ``(beta, group_norms or None, info)``; ``NotImplementedError`` when the problem is not
        one the on-chip solver takes (the caller then runs the sweeps over ``solve_lanes``)."""
        _sync_knobs()
        G = self.n_groups
        a_ = _f64(np.broadcast_to(a, (self.p,)), "a")
        b_ = _f64(np.broadcast_to(b, (G,)), "b")
        b0 = None if beta0 is None else _f64(beta0, "beta0", (self.p,))
        opts = _SolveOpts(float(tol), int(max_iter), 0, 0.0, 0)
        beta = np.empty(self.p)
        gn = np.empty(G) if want_group_norms else None
        info = np.zeros(1, dtype=_INFO_DTYPE)
        _check(
            self._lib.slm_solve_standardized_sgl(
                self._h, _ptr(a_), _ptr(b_), C.byref(opts), float(tol_inner), int(max_sweeps), _ptr(b0), int(bool(warm)),
                _ptr(beta), _ptr(gn), _as(info, _PointInfo),
            )
        )
        return beta, gn, info[0]

    def solve_constrained(self, a, A, lo, hi, beta0=None, warm=False, tol=1e-8, tol_inner=0.0, max_sweeps=0, max_iter=0):
        """``slm_solve_constrained``: ``1/(2n)||X b - y||^2 + sum_j a_j |b_j|`` subject to ``lo <= A b <= hi`` with all
        sweeps of the splitting in one launch.  Returns ``(beta, multipliers, info)``; ``NotImplementedError`` when the
        problem is not one the on-chip solver takes (the caller then runs the sweeps itself, model/_constrained.py)."""
        _sync_knobs()
        a_ = _f64(np.broadcast_to(a, (self.p,)), "a")
        A_ = np.ascontiguousarray(A, dtype=np.float64)
        if A_.ndim != 2 or A_.shape[1] != self.p:
            raise ValueError(f"A must have {self.p} columns")
        m = A_.shape[0]
        lo_ = _f64(lo, "lo", (m,))
        hi_ = _f64(hi, "hi", (m,))
        b0 = None if beta0 is None else _f64(beta0, "beta0", (self.p,))
        opts = _SolveOpts(float(tol), int(max_iter), 0, 0.0, 0)
        beta = np.empty(self.p)
        lam = np.empty(m)
        info = np.zeros(1, dtype=_INFO_DTYPE)
        _check(
            self._lib.slm_solve_constrained(
                self._h, _ptr(a_), _ptr(A_), int(m), _ptr(lo_), _ptr(hi_), C.byref(opts), float(tol_inner), int(max_sweeps),
                _ptr(b0), int(bool(warm)), _ptr(beta), _ptr(lam), _as(info, _PointInfo),
            )
        )
        return beta, lam, info[0]

    # ---- the exact l0 search: what its entries share -------------------------------------------------------------------
    def _need_narrow(self, need):
        """``need`` (one integer mask per group) as the narrow entries take it: one 64-bit word per group."""
        if need is None:
            return None
        need_ = np.ascontiguousarray([int(v) for v in need], dtype=np.uint64)
        if need_.shape != (self.n_groups,):
            raise ValueError(f"need must have {self.n_groups} entries")
        return need_

    def _need_words(self, need):
        """``need`` (one Python integer of up to 128 bits per group) as the wide entries take it: two 64-bit words per group,
        the low one first."""
        if need is None:
            return None
        G = self.n_groups
        vals = [int(v) for v in need]
        if len(vals) != G:
            raise ValueError(f"need must have {G} entries")
        if any(v < 0 or v >> 128 for v in vals):
            raise ValueError("need masks must be non-negative integers of at most 128 bits")
        mask = (1 << 64) - 1
        return np.ascontiguousarray([[v & mask, v >> 64] for v in vals], dtype=np.uint64).reshape(G, 2)

    @staticmethod
    def _l0_route(binding):
        """``binding`` of the l0 methods: None = the compiled binding when it is there, False = ctypes (None is returned),
        True = the binding or an error."""
        b = load_binding() if binding is not False else None
        if binding is True and b is None:
            raise EngineError("the compiled binding is not available")
        return b

    def _l0_call(self, name, binding, args, outs, c_order=None, records=None, binding_args=None):
        """One call of ``slm_<name>`` by the route ``binding`` names.  ``args``: the entry's arguments between the dataset and
        its outputs, arrays as arrays.  ``outs``: the outputs the ctypes route fills -- arrays, ctypes cells, None -- in the
        order of the binding's tuple (``c_order``: their positions in the C signature, where that order differs).  Returns
        ``(outputs, record, rc)``; ``rc`` is ``SLM_OK`` or ``SLM_ERR_NOT_CONVERGED`` (the result is not proven: the outputs
        hold the incumbent), anything else raises.  ``records``: an entry that fills that many records gets them all back
        as an array (None: the one record).  ``binding_args``: the binding's arguments where they differ from ``args`` (an
        entry that takes a list of arrays there and a table of pointers here)."""
        _sync_knobs()
        b = self._l0_route(binding)
        if b is not None:
            *res, rec, rc = getattr(b, name)(self._h.value, self.p, *(args if binding_args is None else binding_args))
            recs = np.frombuffer(rec, dtype=_INFO_DTYPE)
            return res, recs[0] if records is None else recs, rc
        infos = np.zeros(1 if records is None else max(1, records), dtype=_INFO_DTYPE)
        c_outs = [_ptr(o) if o is None or isinstance(o, np.ndarray) else C.byref(o) for o in outs]
        rc = getattr(self._lib, "slm_" + name)(
            self._h, *[_ptr(a) if a is None or isinstance(a, np.ndarray) else a for a in args],
            *[c_outs[i] for i in c_order or range(len(outs))], _as(infos, _PointInfo))
        if rc != SLM_ERR_NOT_CONVERGED:
            _check(rc)
        return [o if o is None or isinstance(o, np.ndarray) else o.value for o in outs], infos[0] if records is None else infos, rc

    @staticmethod
    def _l0_info(info, rc, lower, nodes, *modes):
        """``info`` of a search for one support: the keys every entry reports, from the record's common fields, then what the
        record's other fields mean in each of ``modes`` (the table at ``l0_report``, csrc/engine_l0.hip):
        ``rejects`` counts the descents (``"l1"``) or the qp solves (``"constrained"``), or is the capacity rule's c_min + 1
        (``"wide"``, 0: no include was refused); ``resid`` is 1 where the node budget ran out (``"wide"``) or counts the
        unsettled candidates (``"constrained"``); ``beta_norm`` is the lowest bound on those (``"constrained"``) or the margin
        delta (``"xb"``, where ``mode`` says which bound ran: 5 the exclusion bound, 6 / 7 the plain one)."""
        out = {
            "objective": float(info["kkt"]), "lower_bound": float(lower), "proven_optimal": rc == SLM_OK, "nodes": int(nodes),
            "status": "optimal" if rc == SLM_OK else "node_budget", "loss": float(info["loss"]),
            "seed_objective": float(info["mu"]), "q_all": float(info["L"]), "launches": int(info["n_iter"]),
            "box_tol": 1e-12,  # L0_CD_TOL: relative change per sweep at which boxed candidates' descents stop
        }
        if "l1" in modes:
            out["descents"] = int(info["rejects"])
        if "wide" in modes:
            cut = int(info["rejects"])
            out["capacity_cut"] = cut - 1 if cut else None
            if rc != SLM_OK and float(info["resid"]) == 0.0:
                out["status"] = "capacity"
        if "constrained" in modes:
            unsettled, ubound = int(info["resid"]), float(info["beta_norm"])
            if rc != SLM_OK and unsettled and not out["objective"] <= ubound:
                out["status"] = "unsettled"
            out.update(constrained=True, qp_solves=int(info["rejects"]), unsettled=unsettled, unsettled_bound=ubound,
                       con_tol=1e-9)  # L0_CON_TOL: rows and duality gap of a candidate valued on chip, relative
        if "xb" in modes and int(info["mode"]) == 5:
            out.update(bound="exclusion", bound_margin=float(info["beta_norm"]))
        elif "xb" in modes:
            reason = ("G + 2 eta T is not positive definite on all columns" if int(info["mode"]) == 6 else
                      f"the margin delta = {float(info['beta_norm']):.3g} of the exclusion bound is >= 1/2 (ill-conditioned G + 2 eta T)")
            out.update(bound="q_all", bound_reason=reason)
        return out

    def _l0_search_args(self, wide, alpha, max_groups, eta, T, big_M, need, max_nodes):
        """The arguments ``slm_solve_l0`` and its relatives share, converted."""
        K = self.n_groups if max_groups is None else int(max_groups)
        T_ = None if T is None else _f64(T, "T", (self.p, self.p))
        need_ = self._need_words(need) if wide else self._need_narrow(need)
        return float(alpha), K, float(eta), T_, float(big_M), need_, int(max_nodes)

    def solve_l0_xb(self, alpha=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_xb``: ``solve_l0`` with the exclusion bound -- a subtree is cut against the value on every column the
        path has not excluded, not against the value on all columns (DESIGN 4d "Exclusion bound").  The same arguments and
        result; ``info`` also holds ``bound`` (``"exclusion"``, with ``bound_margin`` = the relative safety margin delta; or
        ``"q_all"`` with ``bound_reason`` when the call fell back to the plain bound: a Gram that is not positive definite on
        all columns, or delta >= 1/2)."""
        return self.solve_l0(alpha, max_groups, eta, T, big_M, need, max_nodes, binding, _xb=True)

    def solve_l0_xb_wide(self, alpha=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_xb_wide``: ``solve_l0_wide`` with the exclusion bound (see ``solve_l0_xb``)."""
        return self.solve_l0_wide(alpha, max_groups, eta, T, big_M, need, max_nodes, binding, _xb=True)

    def solve_l0(self, alpha=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None, _xb=False):
        """``slm_solve_l0``: the exact search over supports of the dataset's groups (csrc/l0_kernels.hpp) for
        ``1/2 b^T (G + 2 eta T) b - c^T b + alpha |S|`` with ``|S| <= max_groups``, ``|b_j| <= big_M`` and the hierarchy
        ``need`` (one integer mask per group).  Returns ``(beta, support mask, info)`` where ``info`` is a dict with
        ``objective``, ``lower_bound``, ``proven_optimal``, ``nodes``, ``status``, ``loss``, ``seed_objective``, ``q_all``,
        ``launches``, ``box_tol``.  ``binding``: None = the compiled binding when it is there, False = ctypes, True = the binding or an
        error (the two routes are compared by the tests)."""
        args = self._l0_search_args(False, alpha, max_groups, eta, T, big_M, need, max_nodes)
        (beta, support, lower, nodes), info, rc = self._l0_call(
            "solve_l0_xb" if _xb else "solve_l0", binding, args, [np.empty(self.p), C.c_uint64(), C.c_double(), C.c_int64()])
        return beta, int(support), self._l0_info(info, rc, lower, nodes, *(("xb",) if _xb else ()))

    def solve_l0_constrained(self, A, lo, hi, alpha=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0,
                             box_lo=None, box_hi=None, max_qp_sweeps=0, m=None, binding=None):
        """``slm_solve_l0_constrained``: ``solve_l0`` subject to ``lo <= A b <= hi`` (``A``: m x p, m <= 64) and the per-column
        box ``box_lo_j <= b_j <= box_hi_j`` (None: ``-big_M`` / ``+big_M``; each interval must contain 0).  ``G + 2 eta T`` must
        be positive definite (``NotImplementedError`` otherwise).  Returns ``(beta, support mask, multipliers, info)``: the
        rows' multipliers (> 0 where ``hi`` binds, < 0 where ``lo`` binds) and ``solve_l0``'s ``info`` with ``qp_solves``
        (candidates valued on chip), ``unsettled`` (candidates whose ``max_qp_sweeps`` sweeps ran out), ``unsettled_bound``
        (the lowest bound on those, ``inf``: none), ``con_tol`` and ``status`` ``"optimal"`` / ``"node_budget"`` /
        ``"unsettled"``; ``q_all`` is the proven lower bound on the value of all columns that the subtree bound used.
        ``m``: the row count handed to the engine (None: ``A``'s)."""
        A_ = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, self.p) if np.size(A) else np.zeros((0, self.p))
        rows = A_.shape[0]
        lo_ = _f64(np.broadcast_to(lo, (rows,)), "lo")
        hi_ = _f64(np.broadcast_to(hi, (rows,)), "hi")
        blo_ = None if box_lo is None else _f64(np.broadcast_to(box_lo, (self.p,)), "box_lo")
        bhi_ = None if box_hi is None else _f64(np.broadcast_to(box_hi, (self.p,)), "box_hi")
        if rows == 0:
            A_ = lo_ = hi_ = None
        args = self._l0_search_args(False, alpha, max_groups, eta, T, big_M, need, max_nodes)
        args += (A_, rows if m is None else int(m), lo_, hi_, blo_, bhi_, int(max_qp_sweeps))
        (beta, support, lam, lower, nodes), info, rc = self._l0_call(
            "solve_l0_constrained", binding, args,
            [np.empty(self.p), C.c_uint64(), np.zeros(rows) if rows else None, C.c_double(), C.c_int64()], c_order=(0, 1, 3, 4, 2))
        lam = np.zeros(0) if lam is None else np.asarray(lam, dtype=np.float64)
        return beta, int(support), lam, self._l0_info(info, rc, lower, nodes, "constrained")

    def solve_l0_l1(self, alpha=0.0, eta_l1=0.0, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_l1``: the exact search in its l1 mode (the reference's ``L1L0``) for
        ``1/2 b^T G b - c^T b + eta_l1 ||b||_1 + alpha |S|`` with ``|b_j| <= big_M`` and the hierarchy ``need``; no bound on
        ``|S|``.  ``eta_l1 == 0`` runs the code of ``solve_l0``.  Returns what ``solve_l0`` returns; ``info`` also holds
        ``descents`` (candidates that passed the lower-bound filter and were valued by the descent) and ``q_all`` is the
        proven lower bound on the value of all columns that the subtree bound used."""
        args = (float(alpha), float(eta_l1), float(big_M), self._need_narrow(need), int(max_nodes))
        (beta, support, lower, nodes), info, rc = self._l0_call(
            "solve_l0_l1", binding, args, [np.empty(self.p), C.c_uint64(), C.c_double(), C.c_int64()])
        return beta, int(support), self._l0_info(info, rc, lower, nodes, "l1")

    def solve_l0_wide(self, alpha=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None, _xb=False):
        """``slm_solve_l0_wide``: ``solve_l0`` on the kernel's wide instantiation -- up to 128 columns and 128 groups, at any
        admissible size (a problem within ``solve_l0``'s limits gives the same bits on either).  ``need`` holds Python
        integers of up to 128 bits and the support comes back as one.  A support holds at most 64 independent columns: an
        include that would bring a 65th is refused, and ``info`` then holds ``capacity_cut`` = the smallest number of groups
        held where that happened (``None``: never) and ``lower_bound <= q_all + alpha (capacity_cut + 1)``.  ``status`` is
        ``"capacity"`` when that alone is why the result is unproven, ``"node_budget"`` when the budget ran out."""
        args = self._l0_search_args(True, alpha, max_groups, eta, T, big_M, need, max_nodes)
        (beta, words, lower, nodes), info, rc = self._l0_call(
            "solve_l0_xb_wide" if _xb else "solve_l0_wide", binding, args,
            [np.empty(self.p), np.zeros(2, dtype=np.uint64), C.c_double(), C.c_int64()])
        support = int(words[0]) | (int(words[1]) << 64)
        return beta, support, self._l0_info(info, rc, lower, nodes, "wide", *(("xb",) if _xb else ()))

    def _l0_profile(self, wide, alpha_min, max_groups, eta, T, big_M, need, max_nodes, binding):
        """Both profile entries: ``(betas, support words, values, info)``."""
        K = self.n_groups if max_groups is None else int(max_groups)
        if K < 0:
            raise ValueError("max_groups must be >= 0")
        args = self._l0_search_args(wide, alpha_min, K, eta, T, big_M, need, max_nodes)
        (betas, supports, values, nodes), info, rc = self._l0_call(
            "solve_l0_profile_wide" if wide else "solve_l0_profile", binding, args,
            [np.empty((K + 1, self.p)), np.empty((K + 1, 2) if wide else K + 1, dtype=np.uint64), np.empty(K + 1), C.c_int64()])
        return betas, supports, values, {
            "nodes": int(nodes), "launches": int(info["n_iter"]), "q_all": float(info["L"]),
            "status": "optimal" if rc == SLM_OK else "node_budget", "proven_optimal": rc == SLM_OK, "box_tol": 1e-12,
        }

    def solve_l0_profile_wide(self, alpha_min=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_profile_wide``: ``solve_l0_profile`` on the kernel's wide instantiation -- up to 128 columns and
        groups, ``max_groups <= 64``, refused (``NotImplementedError``) when the ``max_groups`` largest groups together hold
        more than 64 columns.  ``need`` holds Python integers of up to 128 bits; the support masks come back as a list of
        Python integers (all ones on an entry nobody filled)."""
        betas, words, values, info = self._l0_profile(True, alpha_min, max_groups, eta, T, big_M, need, max_nodes, binding)
        return betas, [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(words).reshape(-1, 2)], values, info

    def solve_l0_profile(self, alpha_min=0.0, max_groups=None, eta=0.0, T=None, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_profile``: one search that returns the best support of EVERY size ``k = 0 .. max_groups`` for
        ``1/2 b^T (G + 2 eta T) b - c^T b`` inside the box and under the hierarchy (the arguments of ``solve_l0``), pruned
        only by what no ``alpha >= alpha_min`` can use.  Returns ``(betas [K + 1, p], support masks [K + 1], values [K + 1],
        info)``; an entry nobody filled holds ``+inf``, an all-ones mask and zeros.  ``info``: ``nodes``, ``launches``,
        ``q_all``, ``status``, ``proven_optimal``, ``box_tol``."""
        return self._l0_profile(False, alpha_min, max_groups, eta, T, big_M, need, max_nodes, binding)

    def _l0_l1_profile(self, wide, alpha_min, max_groups, eta_l1, big_M, need, max_nodes, binding):
        """Both l1 profile entries: ``(betas, support words, values, info)``."""
        K = self.n_groups if max_groups is None else int(max_groups)
        if K < 0:
            raise ValueError("max_groups must be >= 0")
        need_ = self._need_words(need) if wide else self._need_narrow(need)
        args = (float(alpha_min), K, float(eta_l1), float(big_M), need_, int(max_nodes))
        (betas, supports, values, nodes), info, rc = self._l0_call(
            "solve_l0_l1_profile_wide" if wide else "solve_l0_l1_profile", binding, args,
            [np.empty((K + 1, self.p)), np.empty((K + 1, 2) if wide else K + 1, dtype=np.uint64), np.empty(K + 1), C.c_int64()])
        return betas, supports, values, {
            "nodes": int(nodes), "launches": int(info["n_iter"]), "q_all": float(info["L"]), "descents": int(info["rejects"]),
            "status": "optimal" if rc == SLM_OK else "node_budget", "proven_optimal": rc == SLM_OK, "box_tol": 1e-12,
        }

    def solve_l0_l1_profile(self, alpha_min=0.0, max_groups=None, eta_l1=0.0, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_l1_profile``: ``solve_l0_profile`` with an l1 term -- the best support of every size for
        ``min_b 1/2 b^T G b - c^T b + eta_l1 ||b||_1`` inside the box, the table that answers ``solve_l0_l1`` at every
        ``alpha >= alpha_min``.  No ridge term, no ``T``.  Returns what ``solve_l0_profile`` returns; ``info`` also holds
        ``descents`` and ``q_all`` is the proven lower bound on the value of all columns that the subtree cut used.
        ``eta_l1 == 0`` runs the code of ``solve_l0_profile``."""
        return self._l0_l1_profile(False, alpha_min, max_groups, eta_l1, big_M, need, max_nodes, binding)

    def solve_l0_l1_profile_wide(self, alpha_min=0.0, max_groups=None, eta_l1=0.0, big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_l1_profile_wide``: ``solve_l0_l1_profile`` on the kernel's wide instantiation -- up to 128 columns
        and groups, ``max_groups <= 64``, refused (``NotImplementedError``) when the ``max_groups`` largest groups together
        hold more than 64 columns.  Masks as in ``solve_l0_profile_wide``."""
        betas, words, values, info = self._l0_l1_profile(True, alpha_min, max_groups, eta_l1, big_M, need, max_nodes, binding)
        return betas, [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(words).reshape(-1, 2)], values, info

    def solve_l0_profile_batch(self, row_weights, n_effs, intercept=False, alpha_min=0.0, max_groups=None, eta=0.0, T=None,
                               big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_profile_batch``: the tables of ``solve_l0_profile`` for several row sets of this dataset -- the
        training sets of a cross-validation and all rows -- from ONE launch.  ``row_weights``: up to 16 arrays of ``n``
        weights, or None for the dataset's own rows; ``n_effs``: the divisor of each set's Gram (<= 0: the row count).
        ``intercept``: the dataset's last column is a column of ones, alone in the last group; it is not searched but
        eliminated from every set's Gram (weighted centring by the set's own means), so ``T`` is ``ps x ps`` and ``need``
        has one mask per search group, ``ps = p - 1`` columns in ``n_groups - 1`` groups.  ``max_nodes`` is each problem's
        budget.  Returns ``(betas [count, K + 1, ps], intercepts [count, K + 1], support masks [count, K + 1], values
        [count, K + 1], infos)``; ``infos`` is one dict per problem as ``solve_l0_profile`` gives it."""
        return self._l0_profile_rows(row_weights, n_effs, intercept, None, 0, alpha_min, max_groups, eta, T, big_M, need, max_nodes, binding)

    def solve_l0_profile_grid(self, row_weights, n_effs, etas, eta_kind=0, intercept=False, alpha_min=0.0, max_groups=None, T=None,
                              big_M=100.0, need=None, max_nodes=0, binding=None):
        """``slm_solve_l0_profile_grid``: ``solve_l0_profile_batch`` at several weights ``etas`` per row set, from ONE launch.
        ``eta_kind`` 0: ridge weights, every problem is ``solve_l0_profile``'s; 1: l1 weights, every problem is
        ``solve_l0_l1_profile``'s (``T`` must be None).  Problem ``r * len(etas) + e`` is row set ``r`` with ``etas[e]``; at most
        ``L0_GRID_MAX`` = 128 problems.  Returns what ``solve_l0_profile_batch`` returns with the leading dimension
        ``count * len(etas)``; with l1 weights every ``info`` also holds ``descents`` and its ``q_all`` is the l1 lower bound the
        cut used."""
        etas_ = np.ascontiguousarray(etas, dtype=np.float64).reshape(-1)
        return self._l0_profile_rows(row_weights, n_effs, intercept, etas_, int(eta_kind), alpha_min, max_groups, 0.0, T, big_M, need,
                                     max_nodes, binding)

    def _l0_profile_rows(self, row_weights, n_effs, intercept, etas, eta_kind, alpha_min, max_groups, eta, T, big_M, need, max_nodes,
                         binding):
        """Both entries over row sets: ``etas`` None is the batched profile with its one ridge ``eta``, an array the grid."""
        drop = 1 if intercept else 0
        ps, gs = self.p - drop, self.n_groups - drop
        K = gs if max_groups is None else int(max_groups)
        if K < 0:
            raise ValueError("max_groups must be >= 0")
        rws = [None if w is None else _f64(w, "row_weights", (self.n,)) for w in row_weights]
        nes = [int(v) for v in n_effs]
        if len(nes) != len(rws):
            raise ValueError("row_weights and n_effs differ in length")
        count = len(rws)
        T_ = None if T is None else _f64(T, "T", (ps, ps))
        need_ = None
        if need is not None:
            need_ = np.ascontiguousarray([int(v) for v in need], dtype=np.uint64)
            if need_.shape != (gs,):
                raise ValueError(f"need must have {gs} entries")
        ptrs = np.array([0 if w is None else w.ctypes.data for w in rws] or [0], dtype=np.uint64)  # (the table of row-weight pointers)
        ne = np.array(nes or [0], dtype=np.int64)
        if etas is None:
            name, problems = "solve_l0_profile_batch", count
            tail = (bool(intercept), float(alpha_min), K, float(eta), T_, float(big_M), need_, int(max_nodes))
            args = (count, ptrs, ne, int(tail[0])) + tail[1:]
        else:
            name, problems = "solve_l0_profile_grid", count * len(etas)
            if problems > 4 * L0_GRID_MAX:  # (the engine refuses anything above L0_GRID_MAX: the outputs only have to exist)
                problems = 0
            tail = (bool(intercept), etas, eta_kind, float(alpha_min), K, T_, float(big_M), need_, int(max_nodes))
            eta_arr = etas if len(etas) else np.zeros(1)  # (an empty array has no address worth handing over)
            args = (count, ptrs, ne, int(tail[0]), len(etas), eta_arr, eta_kind) + tail[3:]
        cnt = max(1, problems)
        (betas, icpts, supports, values, nodes), infos, rc = self._l0_call(
            name, binding, args,
            [np.empty((cnt, K + 1, ps)), np.empty((cnt, K + 1)), np.empty((cnt, K + 1), dtype=np.uint64), np.empty((cnt, K + 1)),
             np.zeros(cnt, dtype=np.int64)],
            records=problems, binding_args=(self.n, rws, nes) + tail)
        out = [{
            "nodes": int(nodes[b]), "launches": int(infos[b]["n_iter"]), "q_all": float(infos[b]["L"]),
            "status": "optimal" if int(infos[b]["status"]) == SLM_OK else "node_budget",
            "proven_optimal": int(infos[b]["status"]) == SLM_OK, "box_tol": 1e-12,
        } for b in range(problems)]
        if etas is not None and eta_kind == 1:
            for b in range(problems):
                out[b]["descents"] = int(infos[b]["rejects"])
        return betas, icpts, supports, values, out

    def solve_l0_local(self, alphas, etas=0.0, big_M=100.0, starts=None, swaps=True, n_cells=None, n_starts=None, binding=None):
        """``slm_solve_l0_local`` (``swaps=False``: ``slm_solve_l0_local_descent``): the l0 LOCAL SEARCH -- coordinate descent with
        hard thresholding, then one-for-one swaps until none helps (csrc/l0_local_kernels.hpp) -- for
        ``1/2 b^T (G + 2 eta I) b - c^T b + alpha ||b||_0`` with ``|b_j| <= big_M`` at every cell ``(alphas[e], etas[e])``, up
        to 1024 columns, singleton groups.  ``starts``: None (the zero start), or ``[cells, n_starts, p]`` points inside the box;
        every (cell, start) is one problem of ONE launch, and per cell the start with the lowest objective wins.  Nothing is
        proven.  Returns ``(betas [cells, p], objectives [cells], winning starts [cells], infos)``; ``infos`` is one dict per
        cell with ``objective``, ``descent_objective`` (before the host re-solved the winner's support exactly), ``loss``,
        ``sweeps``, ``swaps``, ``converged``, ``status`` (``"fixed_point"``, ``"sweep_cap"``, ``"swap_cap"``) and
        ``proven_optimal`` (False).  ``n_cells`` / ``n_starts``: the counts handed to the engine (None: the arrays')."""
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        st, ns = _l0_local_starts(starts, n_starts, (cells,), self.p, f"cells, n_starts, {self.p}")
        sized = cells >= 1 and ns >= 1 and cells * ns <= L0_LOCAL_MAX_PROBLEMS  # (else the engine refuses: the outputs only have to exist)
        if st is not None and sized and st.size != cells * ns * self.p:
            raise ValueError(f"starts has {st.size} entries, expected {cells * ns * self.p}")
        cnt = cells if sized else 1
        args = (cells, _l0_local_pad(al), _l0_local_pad(et), float(big_M), ns, st if sized else None)
        (betas, objectives, winners), infos, rc = self._l0_call(
            "solve_l0_local" if swaps else "solve_l0_local_descent", binding, args,
            [np.zeros((cnt, self.p)), np.zeros(cnt), np.zeros(cnt, dtype=np.int32)], records=cnt)
        return betas, objectives, winners, _l0_local_infos(infos, cnt)

    def solve_l0_local_folds(self, row_weights, n_effs, alphas, etas=0.0, intercept=False, big_M=100.0, starts=None, swaps=True,
                             n_cells=None, n_starts=None, binding=None):
        """``slm_solve_l0_local_folds``: ``solve_l0_local`` on several row sets of this dataset -- the training sets of a
        cross-validation and all rows -- from ONE launch.  ``row_weights``: up to 16 arrays of ``n`` weights, or None for the
        dataset's own rows; ``n_effs``: the divisor of each set's Gram (<= 0: the row count).  ``intercept``: the dataset's last
        column is a column of ones, alone in the last group; it is not searched but eliminated from every set's Gram (weighted
        centring by the set's own means), so ``ps = p - 1`` columns are searched.  The cells ``(alphas[e], etas[e])`` are shared
        by the row sets; ``starts``: None, or ``[count, cells, n_starts, ps]``.  Returns ``(betas [count, cells, ps], intercepts
        [count, cells], objectives [count, cells], winning starts [count, cells], stats [count, cells, n_starts, 4], infos)``:
        ``stats`` holds sweeps, accepted swaps, status word and non-zeros of EVERY problem; ``infos`` is one list per row set of
        the dicts ``solve_l0_local`` gives per cell.  With one row set of None and no intercept the result equals
        ``solve_l0_local``'s byte for byte."""
        rws, nes = self._l0_local_row_sets(row_weights, n_effs)
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        return self._l0_local_rows("solve_l0_local_folds", 4, rws, nes, al, et, cells, intercept, big_M, starts, swaps, n_starts, binding)

    def solve_l0_local_subsets(self, row_weights, n_effs, sizes, etas=0.0, intercept=False, big_M=100.0, starts=None, swaps=True,
                               n_cells=None, n_starts=None, binding=None):
        """``slm_solve_l0_local_subsets``: LOCAL SUBSETS, the l0 local search in its cardinality form -- for every row set and
        every cell ``(sizes[e], etas[e])`` an approximate minimiser of ``Q = 1/2 b^T (G + 2 eta I) b - c^T b`` over
        ``|b_j| <= big_M`` with at most ``sizes[e]`` non-zeros (shrink, descent on the support, grow, swap scan:
        csrc/l0_local_kernels.hpp), up to 1024 columns, from ONE launch.  Row sets, ``intercept``, ``starts`` (of any support
        size) and the layout of the result as for ``solve_l0_local_folds``; ``[None], [0]`` is the dataset's own rows.
        ``swaps=False`` stops once nothing grows: greedy forward selection with re-fitting.  Returns ``(betas [count, cells,
        ps], intercepts, objectives [count, cells] (Q after the polish), winning starts, stats [count, cells, n_starts, 6],
        infos)``: ``stats`` holds sweeps, accepted swaps, status word, non-zeros, grows and drops of EVERY problem; ``infos``
        the dicts of ``solve_l0_local`` with ``grows`` and ``drops`` of the winner beside them.  Nothing is proven."""
        rws, nes = self._l0_local_row_sets(row_weights, n_effs)
        sz = None
        if sizes is not None:  # (None reaches the engine as NULL, by the ctypes route: its first refusal)
            raw = np.asarray(sizes).reshape(-1)
            if raw.size and not np.all(np.isfinite(raw.astype(np.float64)) & (raw == np.floor(raw)) & (np.abs(raw) < 2 ** 31)):
                raise ValueError("sizes must be integers")
            sz = np.ascontiguousarray(raw, dtype=np.int32)
        if etas is None or sz is None:
            et = None if etas is None else np.ascontiguousarray(np.atleast_1d(etas), dtype=np.float64).reshape(-1)
        else:
            et = np.ascontiguousarray(np.broadcast_to(np.asarray(etas, dtype=np.float64), sz.shape), dtype=np.float64).reshape(-1)
        given = [len(v) for v in (sz, et) if v is not None]
        cells = (min(given) if given else 1) if n_cells is None else int(n_cells)
        if any(g < cells for g in given):
            raise ValueError("sizes and etas must have n_cells entries")
        return self._l0_local_rows("solve_l0_local_subsets", 6, rws, nes, sz, et, cells, intercept, big_M, starts, swaps, n_starts, binding)

    def solve_l0_local_groups(self, row_weights, n_effs, alphas, etas=0.0, need=None, intercept=False, big_M=100.0, starts=None,
                              swaps=True, n_cells=None, n_starts=None, binding=None):
        """``slm_solve_l0_local_groups``: the l0 local search WITH GROUPS AND A HIERARCHY (csrc/l0_local_group_kernels.hpp) --
        ``1/2 b^T (G + 2 eta I) b - c^T b + alpha |cl(S(b))|`` with ``|b_j| <= big_M``, ``S`` the groups that hold a non-zero, ``cl``
        the closure under the hierarchy -- on the dataset's groups (``set_groups``), which must be contiguous and ascending in
        column order.  ``need``: None, one list per search group of the groups it needs directly (the engine closes them
        transitively), or the CSR pair ``(need_ptr, need_idx)`` as it goes to the engine.  Row sets, ``intercept`` (the ones column
        and its group are not searched), cells, ``starts`` and ``swaps`` as for ``solve_l0_local_folds``.  Returns ``(betas [count,
        cells, ps], intercepts, objectives [count, cells], winning starts, group supports [count, cells, groups] (cl(S), int32),
        stats [count, cells, n_starts, 6], infos)``: ``stats`` holds sweeps, accepted swaps, status word, |cl(S)|, non-zero
        columns and group trials of EVERY problem; ``infos`` the dicts of ``solve_l0_local`` with ``n_active_groups`` and ``trials``
        of the winner.  Nothing is proven, and the screen of the group descent is a heuristic."""
        rws, nes = self._l0_local_row_sets(row_weights, n_effs)
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        drop = 1 if intercept else 0
        ps, gs, count = self.p - drop, max(self.n_groups - drop, 0), len(rws)
        ptr, idx = _l0_need_csr(need, gs)
        st, ns = _l0_local_starts(starts, n_starts, (count, cells), ps, f"{count}, {cells}, n_starts, {ps}")
        # (else the engine refuses: the outputs only have to exist)
        sized = 1 <= count <= 16 and cells >= 1 and ns >= 1 and cells * ns <= L0_LOCAL_MAX_PROBLEMS and count * cells * ns <= L0_LOCAL_MAX_PROBLEMS
        if st is not None and sized and st.size != count * cells * ns * ps:
            raise ValueError(f"starts has {st.size} entries, expected {count * cells * ns * ps}")
        cnt = count * cells if sized else 1
        problems = cnt * ns if sized else 1
        ptrs = np.array([0 if w is None else w.ctypes.data for w in rws] or [0], dtype=np.uint64)  # (the table of row-weight pointers)
        ne = np.array(nes or [0], dtype=np.int64)
        tail = (int(bool(intercept)), cells, _l0_local_pad(al), _l0_local_pad(et), float(big_M), ptr, idx, ns, st if sized else None,
                int(bool(swaps)))
        (betas, icpts, objectives, winners, gsup, stats), infos, rc = self._l0_call(
            "solve_l0_local_groups", binding, (count, ptrs, ne) + tail,
            [np.zeros((cnt, ps)), np.zeros(cnt), np.zeros(cnt), np.zeros(cnt, dtype=np.int32), np.zeros((cnt, max(gs, 1)), dtype=np.int32),
             np.zeros((problems, 6), dtype=np.int32)],
            records=cnt, binding_args=(self.n, self.n_groups, rws, nes, bool(intercept)) + tail[1:-1] + (bool(swaps),))
        out = _l0_local_infos(infos, cnt)
        if not sized:
            return betas, icpts, objectives, winners, gsup, stats, [out]
        stats = stats.reshape(count, cells, ns, 6)
        for e in range(cnt):
            won = stats[e // cells, e % cells, int(winners[e])]
            out[e]["n_active_groups"], out[e]["trials"] = int(np.count_nonzero(gsup[e][:gs])), int(won[5])
        return (betas.reshape(count, cells, ps), icpts.reshape(count, cells), objectives.reshape(count, cells), winners.reshape(count, cells),
                gsup[:, :gs].reshape(count, cells, gs), stats, [out[r * cells:(r + 1) * cells] for r in range(count)])

    def solve_l0_local_l1(self, row_weights, n_effs, alphas, l1s, ridges=0.0, intercept=False, big_M=100.0, starts=None, swaps=True,
                          n_cells=None, n_starts=None, binding=None):
        """``slm_solve_l0_local_l1``: the l0 local search WITH AN L1 TERM (``l0_local_l1_kernel``, csrc/l0_local_kernels.hpp) --
        ``1/2 b^T (G + 2 ridge I) b - c^T b + l1 ||b||_1 + alpha ||b||_0`` with ``|b_j| <= big_M`` at every cell ``(alphas[e],
        l1s[e], ridges[e])``: with ``ridge = 0`` the objective of ``solve_l0_l1`` (the reference's ``L1L0``) with singleton groups,
        for up to 1024 columns.  ``l1s``, ``ridges``: scalars or one value per cell; ``ridges=None`` reaches the engine as NULL
        (no ridge).  Row sets, ``intercept``, ``starts``, ``swaps`` and the layout of the result as for ``solve_l0_local_folds``:
        ``(betas [count, cells, ps], intercepts, objectives, winning starts, stats [count, cells, n_starts, 4], infos)``.  The
        winner is polished on its support (soft-threshold descent, then the exact solve on its sign pattern); a coefficient the
        polish brings to zero comes back as zero.  With every ``l1s[e] = 0`` the decisions are ``solve_l0_local_folds``'s.  Nothing
        is proven."""
        rws, nes = self._l0_local_row_sets(row_weights, n_effs)
        al = None if alphas is None else np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        shape = (1,) if al is None else al.shape

        def per_cell(v):  # (None reaches the engine as NULL, by the ctypes route)
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape), dtype=np.float64).reshape(-1)

        l1, rd = per_cell(l1s), per_cell(ridges)
        given = [len(v) for v in (al, l1, rd) if v is not None]
        cells = (min(given) if given else 1) if n_cells is None else int(n_cells)
        if any(g < cells for g in given):
            raise ValueError("alphas, l1s and ridges must have n_cells entries")
        return self._l0_local_rows("solve_l0_local_l1", 4, rws, nes, al, rd, cells, intercept, big_M, starts, swaps, n_starts, binding,
                                   between=(l1,), optional_et=True)

    def solve_l0_local_bound(self, alphas, etas=0.0, big_M=100.0, starts=None, max_sweeps=0, gap_tol=1e-9, n_cells=None, binding=None):
        """``slm_solve_l0_local_bound``: the LOCAL BOUND (``l0_local_bound_kernel``, csrc/l0_local_bound_kernels.hpp) -- for every
        cell ``(alphas[e], etas[e])`` a PROVEN lower bound on ``min 1/2 b^T (G + 2 eta I) b - c^T b + alpha ||b||_0`` over
        ``|b_j| <= big_M``, the objective ``solve_l0_local`` minimises, up to 1024 columns, singleton groups, one launch.  The bound
        is ``L(u) = -1/2 u^T G u - sum_j max(0, h(c_j - (G u)_j) - alpha)``, valid for every ``u``; the kernel looks for the
        tightest one by coordinate descent on the convex relaxation from ``starts`` (None, or ``[cells, p]``, clipped into the
        box) and stops a cell at a relative gap of ``gap_tol`` or after ``max_sweeps`` sweeps (<= 0: 10000).  Tight with a ridge
        or a box that binds, weak at ``eta = 0`` under a loose ``big_M``.  Returns ``(bounds [cells], relaxed objectives [cells],
        u [cells, p], stats [cells, 2] (sweeps, status word), infos)``; ``infos`` is one dict per cell with ``lower_bound``,
        ``relaxed_objective``, ``sweeps``, ``converged``, ``status`` (``"closed"``, ``"sweep_cap"``) and ``call_status`` (what the
        call returned: ``SLM_OK``, or ``SLM_ERR_NOT_CONVERGED`` when some cell ran out of sweeps).  The values are bounds whatever
        the status."""
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        sized = 1 <= cells <= L0_LOCAL_MAX_PROBLEMS  # (else the engine refuses: the outputs only have to exist)
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1)
        if st is not None and sized and st.size != cells * self.p:
            raise ValueError(f"starts has {st.size} entries, expected {cells * self.p}")
        cnt = cells if sized else 1
        args = (cells, _l0_local_pad(al), _l0_local_pad(et), float(big_M), st if sized else None, int(max_sweeps), float(gap_tol))
        (lower, primal, u, stats), infos, rc = self._l0_call(
            "solve_l0_local_bound", binding, args,
            [np.zeros(cnt), np.zeros(cnt), np.zeros((cnt, self.p)), np.zeros((cnt, 2), dtype=np.int32)], records=cnt)
        out = [{"lower_bound": float(infos[e]["L"]), "relaxed_objective": float(infos[e]["mu"]), "sweeps": int(infos[e]["n_iter"]),
                "converged": int(infos[e]["status"]) == SLM_OK, "status": "closed" if int(infos[e]["resid"]) == 0 else "sweep_cap",
                "call_status": int(rc)} for e in range(cnt)]
        return lower, primal, u, stats, out

    def solve_l0_local_group_nodes(self, alphas, etas, cell, in_mask, out_mask, need=None, big_M=100.0, parent_lower=None, starts=None,
                                   max_sweeps=0, gap_tol=1e-9, n_cells=None):
        """``slm_solve_l0_local_group_nodes``: ONE BATCH of GROUP node relaxations of the local proof with groups
        (``l0_local_group_node_kernel``, csrc/l0_local_group_node_kernels.hpp).  As ``solve_l0_local_nodes``, with the masks BY
        GROUP (bit ``g & 63`` of word ``g >> 6``: group ``g`` of the dataset's contiguous, ascending groups) and ``need`` as for
        ``solve_l0_local_groups``; ``upper = F(u)`` counts ``|cl(S(u))|``.  Masks that are not closed under the hierarchy are
        refused."""
        return self.solve_l0_local_nodes(alphas, etas, cell, in_mask, out_mask, big_M, parent_lower, starts, max_sweeps, gap_tol, n_cells,
                                         _need=_l0_need_csr(need, self.n_groups))

    def solve_l0_local_group_prove(self, alphas, etas=0.0, need=None, big_M=100.0, incumbents=None, rel_gap=1e-6, max_nodes=20000, width=32,
                                   max_sweeps=0, leaf_capacity=0, n_cells=None):
        """``slm_solve_l0_local_group_prove``: THE LOCAL PROOF WITH GROUPS AND A HIERARCHY -- branch and bound over group nodes for
        ``slm_solve_l0_local_groups``' objective.  As ``solve_l0_local_prove``, with ``need`` as for ``solve_l0_local_groups``; the
        dict gains ``group_support`` (``[cells, groups]`` int32: cl(S) of the incumbents) and the leaves' masks are group masks."""
        return self.solve_l0_local_prove(alphas, etas, big_M, incumbents, rel_gap, max_nodes, width, max_sweeps, leaf_capacity, n_cells,
                                         _need=_l0_need_csr(need, self.n_groups))

    def solve_l0_local_nodes(self, alphas, etas, cell, in_mask, out_mask, big_M=100.0, parent_lower=None, starts=None, max_sweeps=0,
                             gap_tol=1e-9, n_cells=None, _need=None):
        """``slm_solve_l0_local_nodes``: ONE BATCH of node relaxations of the local proof (``l0_local_node_kernel``,
        csrc/l0_local_node_kernels.hpp), one wavefront per node, one launch.  Node ``i`` belongs to cell ``cell[i]`` of
        ``(alphas, etas)``; ``in_mask[i]`` and ``out_mask[i]`` are 16 words of 64 bits each (bit ``j & 63`` of word ``j >> 6``:
        column ``j`` is fixed IN, or OUT; neither: FREE).  ``parent_lower`` (None, or ``[nodes]``) is folded into the bound,
        ``starts`` (None, or ``[nodes, p]``) is clipped into the box.  Returns ``(lower [nodes], primal [nodes], upper [nodes],
        u [nodes, p], stats [nodes, 2] (sweeps, status word), call_status)``: ``lower`` is a proven bound of the node whatever the
        status, ``upper = F(u)`` an upper bound of the cell."""
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        ce = np.ascontiguousarray(cell, dtype=np.int32).reshape(-1)
        nodes = len(ce)
        im = np.ascontiguousarray(in_mask, dtype=np.uint64).reshape(-1)
        om = np.ascontiguousarray(out_mask, dtype=np.uint64).reshape(-1)
        if im.size != 16 * nodes or om.size != 16 * nodes:
            raise ValueError(f"in_mask and out_mask must hold 16 words per node ({16 * nodes}), got {im.size} and {om.size}")
        pl = None if parent_lower is None else np.ascontiguousarray(parent_lower, dtype=np.float64).reshape(-1)
        if pl is not None and pl.size != nodes:
            raise ValueError(f"parent_lower has {pl.size} entries, expected {nodes}")
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1)
        if st is not None and st.size != nodes * self.p:
            raise ValueError(f"starts has {st.size} entries, expected {nodes * self.p}")
        cnt = max(1, nodes)
        args = (cells, _l0_local_pad(al), _l0_local_pad(et), float(big_M), nodes, _l0_local_pad(ce), _l0_local_pad(im), _l0_local_pad(om), pl, st,
                *(() if _need is None else _need), int(max_sweeps), float(gap_tol))  # (_need: the grouped entry, with its two lists)
        (lower, primal, upper, u, stats), _, rc = self._l0_call(
            "solve_l0_local_nodes" if _need is None else "solve_l0_local_group_nodes", False, args,
            [np.zeros(cnt), np.zeros(cnt), np.zeros(cnt), np.zeros((cnt, self.p)), np.zeros((cnt, 2), dtype=np.int32)], records=cnt)
        return lower, primal, upper, u, stats, int(rc)

    def solve_l0_local_prove(self, alphas, etas=0.0, big_M=100.0, incumbents=None, rel_gap=1e-6, max_nodes=20000, width=32, max_sweeps=0,
                             leaf_capacity=0, n_cells=None, _need=None):
        """``slm_solve_l0_local_prove``: THE LOCAL PROOF -- branch and bound on the local bound for every cell ``(alphas[e], etas[e])``,
        one launch of ``l0_local_node_kernel`` a round for the children of every cell.  ``incumbents``: None, or ``[cells, p]`` inside
        the box.  ``leaf_capacity > 0`` asks for the certificate: every dropped node's cell, masks, u and bound.  Returns a dict:
        ``beta [cells, p]``, ``objective``, ``lower_bound``, ``nodes``, ``rounds``, ``status`` (0: proven optimal to ``rel_gap``; 1:
        the node limit), ``call_status`` and, with a capacity, ``leaves`` (``cell``, ``in_mask``, ``out_mask``, ``u``, ``lower``,
        ``count``: all dropped nodes, of which the arrays hold the first ``leaf_capacity``).  The tree closes with a ridge or a box
        that binds; at ``eta = 0`` with more columns than rows it does not, and ``lower_bound`` is what was proven."""
        al, et, cells = _l0_local_cells(alphas, etas, n_cells)
        sized = 1 <= cells <= L0_LOCAL_MAX_PROBLEMS
        inc = None if incumbents is None else np.ascontiguousarray(incumbents, dtype=np.float64).reshape(-1)
        if inc is not None and sized and inc.size != cells * self.p:
            raise ValueError(f"incumbents has {inc.size} entries, expected {cells * self.p}")
        cnt, cap = (cells if sized else 1), max(0, int(leaf_capacity))
        lc = C.c_int64(0)
        leaf = [np.zeros(max(1, cap), dtype=np.int32), np.zeros((max(1, cap), 16), dtype=np.uint64), np.zeros((max(1, cap), 16), dtype=np.uint64),
                np.zeros((max(1, cap), self.p)), np.zeros(max(1, cap))]
        args = (cells, _l0_local_pad(al), _l0_local_pad(et), float(big_M), inc if sized else None, *(() if _need is None else _need),
                float(rel_gap), int(max_nodes), int(width), int(max_sweeps), cap)  # (_need: the grouped entry, with its two lists)
        gsup = [] if _need is None else [np.zeros((cnt, max(self.n_groups, 1)), dtype=np.int32)]
        outs = [np.zeros((cnt, self.p)), np.zeros(cnt), np.zeros(cnt), np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.int32),
                np.zeros(cnt, dtype=np.int32), *gsup, *leaf, lc]
        (beta, obj, low, nodes, rounds, status, *_), _, rc = self._l0_call(
            "solve_l0_local_prove" if _need is None else "solve_l0_local_group_prove", False, args, outs, records=cnt)
        out = {"beta": beta, "objective": obj, "lower_bound": low, "nodes": nodes, "rounds": rounds, "status": status, "call_status": int(rc)}
        if gsup:
            out["group_support"] = gsup[0][:, :self.n_groups]
        if cap:
            k = min(cap, int(lc.value))
            out["leaves"] = {"cell": leaf[0][:k], "in_mask": leaf[1][:k], "out_mask": leaf[2][:k], "u": leaf[3][:k], "lower": leaf[4][:k],
                             "count": int(lc.value)}
        return out

    def _l0_local_row_sets(self, row_weights, n_effs):
        """The row sets of a local-search call: ``(the weight arrays or None, the divisors)``, one per set."""
        rws = [None if w is None else _f64(w, "row_weights", (self.n,)) for w in row_weights]
        nes = [int(v) for v in n_effs]
        if len(nes) != len(rws):
            raise ValueError("row_weights and n_effs differ in length")
        return rws, nes

    def _l0_local_rows(self, name, nstat, rws, nes, first, et, cells, intercept, big_M, starts, swaps, n_starts, binding, between=(),
                       optional_et=False):
        """The entries over row sets.  ``first``: the cells' alphas (``nstat`` 4 status words per problem) or their sizes (6:
        grows and drops behind the four), coerced by the caller; a None there or in ``et`` reaches the engine as NULL.
        ``between``: per-cell arrays the entry takes between ``first`` and ``et`` (the l1 entry's l1 weights); ``optional_et``: the
        entry takes a NULL there by either route."""
        ps, count = self.p - (1 if intercept else 0), len(rws)
        st, ns = _l0_local_starts(starts, n_starts, (count, cells), ps, f"{count}, {cells}, n_starts, {ps}")
        # (else the engine refuses: the outputs only have to exist)
        sized = 1 <= count <= 16 and cells >= 1 and ns >= 1 and cells * ns <= L0_LOCAL_MAX_PROBLEMS and count * cells * ns <= L0_LOCAL_MAX_PROBLEMS
        if st is not None and sized and st.size != count * cells * ns * ps:
            raise ValueError(f"starts has {st.size} entries, expected {count * cells * ns * ps}")
        cnt = count * cells if sized else 1
        problems = cnt * ns if sized else 1
        ptrs = np.array([0 if w is None else w.ctypes.data for w in rws] or [0], dtype=np.uint64)  # (the table of row-weight pointers)
        ne = np.array(nes or [0], dtype=np.int64)
        tail = ((int(bool(intercept)), cells, _l0_local_pad(first)) + tuple(_l0_local_pad(v) for v in between)
                + (_l0_local_pad(et), float(big_M), ns, st if sized else None, int(bool(swaps))))
        if first is None or (et is None and not optional_et) or any(v is None for v in between):
            binding = False  # (the compiled route takes arrays: a NULL goes by ctypes)
        (betas, icpts, objectives, winners, stats), infos, rc = self._l0_call(
            name, binding, (count, ptrs, ne) + tail,
            [np.zeros((cnt, ps)), np.zeros(cnt), np.zeros(cnt), np.zeros(cnt, dtype=np.int32), np.zeros((problems, nstat), dtype=np.int32)],
            records=cnt, binding_args=(self.n, rws, nes, bool(intercept)) + tail[1:-1] + (bool(swaps),))
        out = _l0_local_infos(infos, cnt)
        if not sized:
            return betas, icpts, objectives, winners, stats, [out]
        stats = stats.reshape(count, cells, ns, nstat)
        for e in range(cnt if nstat == 6 else 0):
            won = stats[e // cells, e % cells, int(winners[e])]
            out[e]["grows"], out[e]["drops"] = int(won[4]), int(won[5])
        return (betas.reshape(count, cells, ps), icpts.reshape(count, cells), objectives.reshape(count, cells), winners.reshape(count, cells),
                stats, [out[r * cells:(r + 1) * cells] for r in range(count)])


def _l0_need_csr(need, gs):
    """The need lists of ``gs`` groups as the engine takes them, ``(need_ptr, need_idx)``: from None (no hierarchy: two NULLs), one
    list per group, or the CSR pair itself."""
    if need is None:
        return None, None
    if isinstance(need, tuple):
        ptr, idx = (None if v is None else np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in need)
        if ptr is None or len(ptr) != gs + 1:
            raise ValueError(f"need_ptr must have {gs + 1} entries")
        if idx is not None and len(ptr) and len(idx) < max(int(ptr.max()), 0):
            raise ValueError("need_idx is shorter than need_ptr says")
    else:
        lists = [np.asarray(v, dtype=np.int64).reshape(-1) for v in need]
        if len(lists) != gs:
            raise ValueError(f"need must have {gs} entries")
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
        idx = np.ascontiguousarray(np.concatenate(lists + [np.zeros(0, dtype=np.int64)]), dtype=np.int32)
    if idx is not None and not len(idx):
        idx = np.zeros(1, dtype=np.int32)  # (an empty array has no address worth handing over)
    return ptr, idx


def _l0_local_cells(alphas, etas, n_cells):
    """The cells of the penalised local search as the engine takes them: ``(alphas, etas, the count handed over)``."""
    al = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
    et = np.ascontiguousarray(np.broadcast_to(np.asarray(etas, dtype=np.float64), al.shape), dtype=np.float64).reshape(-1)
    cells = len(al) if n_cells is None else int(n_cells)
    if len(al) < cells or len(et) < cells:
        raise ValueError("alphas and etas must have n_cells entries")
    return al, et, cells


def _l0_local_starts(starts, n_starts, lead, width, shape_text):
    """``(starts flat or None, the start count)``.  Without ``n_starts`` the array must be ``lead + (n_starts, width)``."""
    if starts is None:
        return None, 1 if n_starts is None else int(n_starts)
    st = np.ascontiguousarray(starts, dtype=np.float64)
    if n_starts is not None:
        return st.reshape(-1), int(n_starts)
    if st.ndim != len(lead) + 2 or st.shape[:-2] != tuple(lead) or st.shape[-1] != width:
        raise ValueError(f"starts must have the shape ({shape_text})")
    return st.reshape(-1), st.shape[-2]


def _l0_local_pad(v):
    """An empty array has no address worth handing over: one zero of its type instead.  (None stays None: a NULL.)"""
    return v if v is None or len(v) else np.zeros(1, dtype=v.dtype)


def _l0_local_infos(infos, cnt):
    """The dict per (row set,) cell of the local-search wrappers, from the engine's records."""
    names = {0: "fixed_point", 1: "sweep_cap", 2: "swap_cap", 3: "sweep_cap"}
    return [{
        "objective": float(infos[e]["kkt"]), "descent_objective": float(infos[e]["mu"]), "loss": float(infos[e]["loss"]),
        "sweeps": int(infos[e]["n_iter"]), "swaps": int(infos[e]["rejects"]), "converged": int(infos[e]["status"]) == SLM_OK,
        "status": names.get(int(infos[e]["resid"]), "sweep_cap"), "proven_optimal": False, "launches": 1,
    } for e in range(cnt)]


class _HostPool:
    """Result buffers in page-locked host memory (``slm_host_alloc``), recycled.

    The engine copies coefficients straight into whatever host pointer it is given.  Into ordinary numpy memory the
    HIP runtime locks the pages first and remembers them; when numpy later frees such an array (a 2 MB path result,
    32 MB for sixteen lanes) the driver has to tear that registration down, which now and then stalled the NEXT
    solve's first submissions for 20 ms (bench.py's config-4 leg: 0.25 s instead of 0.16 s).  Blocks from this pool
    are never unmapped while the process lives: an array handed out keeps its block until the last view of it is
    gone (``weakref.finalize`` on the exporting buffer), then the block goes back on the free list of its size
    class (powers of two from 64 KiB).  At most ``cap`` bytes sit idle; anything beyond goes back to the driver.
    Small results, and everything after a fork, use plain numpy memory."""

    MIN_BYTES = 1 << 16

    def __init__(self, cap=1 << 30):
        self.cap, self.idle = cap, 0
        self.free: dict[int, list[int]] = {}
        # (re-entrant: `_give` runs from weakref.finalize, which a garbage collection inside `_take` / `_give` -- while
        #  the lock is held -- can trigger on this very thread)
        self.lock = threading.RLock()
        self.pid = os.getpid()

    def _take(self, size):
        with self.lock:
            blocks = self.free.get(size)
            if blocks:
                self.idle -= size
                return blocks.pop()
        ptr = C.c_void_p()
        rc = load_library().slm_host_alloc(C.c_size_t(size), C.byref(ptr))
        return ptr.value if rc == 0 and ptr.value else None

    def _give(self, ptr, size, pid):
        if pid != os.getpid() or _lib is None:  # (a forked child, or the library is already gone at exit)
            return
        with self.lock:
            if self.idle + size <= self.cap:
                self.free.setdefault(size, []).append(ptr)
                self.idle += size
                return
        try:
            _lib.slm_host_free(C.c_void_p(ptr))
        except Exception:  # interpreter shutdown
            pass

    def empty(self, n_doubles: int) -> np.ndarray:
        """Uninitialised float64 vector of `n_doubles` entries."""
        nbytes = 8 * int(n_doubles)
        if nbytes < self.MIN_BYTES or os.getpid() != self.pid or os.environ.get("SLM_NO_HOST_POOL"):
            return np.empty(int(n_doubles))
        size = 1 << (nbytes - 1).bit_length()
        ptr = self._take(size)
        if ptr is None:  # no page-locked memory to be had: ordinary memory works too
            return np.empty(int(n_doubles))
        buf = (C.c_char * size).from_address(ptr)
        weakref.finalize(buf, self._give, ptr, size, self.pid)
        return np.frombuffer(buf, dtype=np.float64, count=int(n_doubles))


_host_pool = _HostPool()


def init_local_comm(engines, timeout_s: float = 0.0) -> None:
    """Make ``engines`` (same process, same device, one host thread each) the ranks of a row-sharded job."""
    lib = load_library()
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    _check(lib.slm_comm_init_local(arr, len(engines), float(timeout_s)))


# -- default engine per process / device ------------------------------------------------------------
_engines: dict[tuple[int, int], Engine] = {}
_engines_lock = threading.Lock()


def _close_engines():
    with _engines_lock:
        pid = os.getpid()
        _engines.clear()
    for eng in list(_live_engines):
        if eng._pid == pid:  # (a forked child never touches its parent's handles)
            eng.close()


import atexit  # noqa: E402

atexit.register(_close_engines)


# The library reads the SLM_* environment variables once.  The Python layer notices when one of them changes afterwards
# (os.environ[...] = ..., del os.environ[...], pytest's monkeypatch.setenv: all raise the audit events os.putenv /
# os.unsetenv BEFORE the change lands) and has the library read them again at the next call into it -- so tests and tools
# that flip a knob mid-process keep working without calling reload_knobs() themselves.
_knobs_dirty = False


def _env_audit(event, args):
    global _knobs_dirty
    if event == "os.putenv" or event == "os.unsetenv":
        key = args[0]
        if (isinstance(key, bytes) and key.startswith(b"SLM_")) or (isinstance(key, str) and key.startswith("SLM_")):
            _knobs_dirty = True


sys.addaudithook(_env_audit)


def _sync_knobs() -> None:
    global _knobs_dirty
    if _knobs_dirty:
        _knobs_dirty = False
        reload_knobs()


def reload_knobs() -> None:
    """Have the library read the SLM_* environment variables again (it reads them once, when it first needs one): for tests
    and tools that change a variable after the library was loaded."""
    _check(load_library().slm_reload_knobs())


def get_engine(device_id: int | None = None) -> Engine:
    """Process-wide engine for ``device_id`` (default: ``LOCAL_RANK`` or 0).  Fork-safe by keying on pid."""
    if device_id is None:
        device_id = int(os.environ.get("SLM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = device_count()
        if n > 0:
            device_id %= n
    key = (os.getpid(), int(device_id))
    with _engines_lock:
        eng = _engines.get(key)
        if eng is None:
            eng = Engine(device_id)
            _engines[key] = eng
        return eng
