"""ctypes binding of the C ABI (`include/relp_engine.h`, built into `librelp_engine.so`) and the
host-side mirror of the reference interface for the pivot path.

Names follow the reference (file:line under /root/reference/src/algorithm/two_phase/):
  ``Tableau``            tableau/mod.rs:24 -- relative_cost(s), generate_column, generate_element,
                         select_primal_pivot_row, bring_into_basis, current_bfs, objective_function_value
  ``PivotRule`` values   strategy/pivot_rule.rs:38,62,97
  ``phase_one_primal`` / ``phase_two_primal`` / ``solve_relaxation``
                         phase_one.rs:125, phase_two.rs:22, two_phase/mod.rs:30

The HIP library is mandatory.  If it is missing or fails to load this module raises: there is no
CPU fallback (the CPU restatements live in ``oracle/`` and are test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np

from .matrix_data import MatrixData

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librelp_engine.so")

# relp_pivot_rule_t
FIRST_PROFITABLE, FIRST_PROFITABLE_WITH_MEMORY, STEEPEST_DESCENT = 0, 1, 2
# relp_outcome_t
RUNNING, OPTIMAL, UNBOUNDED, INFEASIBLE, PHASE_ONE_DONE, NO_ROW_PHASE_ONE = range(6)
# kind of relp_gomory_cuts, and its status per list entry
GOMORY_FRACTIONAL, GOMORY_MIXED = 0, 1
GOMORY_CUT, GOMORY_NOT_INTEGER, GOMORY_FRACTION, GOMORY_ARTIFICIAL, GOMORY_CONTINUOUS = range(5)
# status of relp_strong_branch per list entry
BRANCH_EVALUATED, BRANCH_NOT_STRUCTURAL, BRANCH_FRACTION = range(3)
OUTCOME_NAMES = {RUNNING: "running", OPTIMAL: "optimal", UNBOUNDED: "unbounded", INFEASIBLE: "infeasible",
                 PHASE_ONE_DONE: "phase_one_done", NO_ROW_PHASE_ONE: "no_row_phase_one"}
# relp_kernel_id_t
(K_PRICE, K_SELECT_COLUMN, K_BUILD_COLUMN, K_FTRAN, K_RATIO, K_UPDATE_VECTORS, K_UPDATE_INVERSE, K_APPLY_W,
 K_UPDATE_W, K_FLUSH, K_FT_RUN) = range(11)
KERNEL_NAMES = ["price", "select_column", "build_column", "ftran", "ratio", "update_vectors", "update_inverse",
                "apply_w", "update_w", "flush", "ft_run"]
ENGINE_REVISED, ENGINE_TABLEAU, ENGINE_LU, ENGINE_AUTO = 0, 1, 2, 3   # relp_engine_kind_t
RATIO_REFERENCE, RATIO_LARGEST_PIVOT = 0, 1           # relp_ratio_rule_t (f64 safeguard; 0 = tableau/mod.rs:229-239)
ARTIFICIAL_REFERENCE, ARTIFICIAL_TEXTBOOK = 0, 1      # relp_artificial_removal_t (0 = phase_one.rs:223-260 literally)
# relp_status_t
E_ARG, E_HIP, E_ZERO_PIVOT, E_SINGULAR, E_STATE, E_UNSUPPORTED, E_ALLOC = -1, -2, -3, -4, -5, -6, -7
FORMAT_CSC, FORMAT_DENSE = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1


class RelpError(RuntimeError):
    pass


class _MatrixData(C.Structure):
    _fields_ = [("nr_normal", C.c_int32), ("nr_eq", C.c_int32), ("nr_range", C.c_int32), ("nr_le", C.c_int32),
                ("nr_ge", C.c_int32), ("format", C.c_int32), ("matrix_memory", C.c_int32),
                ("col_ptr", C.c_void_p), ("row_idx", C.c_void_p), ("values", C.c_void_p),
                ("dense", C.c_void_p), ("dense_ld", C.c_int64),
                ("b", C.c_void_p), ("ranges", C.c_void_p), ("cost", C.c_void_p), ("upper_bound", C.c_void_p)]


class Config(C.Structure):
    """relp_config_t"""
    _fields_ = [("device", C.c_int32), ("phase_one_rule", C.c_int32), ("phase_two_rule", C.c_int32),
                ("tol_cost", C.c_double), ("tol_pivot", C.c_double), ("tol_zero", C.c_double),
                ("tol_tie", C.c_double), ("tol_feas", C.c_double),
                ("poll_interval", C.c_int32), ("trace_capacity", C.c_int32),
                ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("update_block", C.c_int32), ("engine", C.c_int32),
                ("ratio_rule", C.c_int32), ("artificial_removal", C.c_int32),
                ("pivot_rescue", C.c_int32), ("auto_reinversion", C.c_int32)]


# every symbol include/relp_engine.h declares (tests/test_abi.py checks the export list against the header)
_SIGNATURES = {
    "relp_default_config": (None, [C.POINTER(Config)]),
    "relp_robust_config": (None, [C.POINTER(Config)]),
    "relp_engine_kind": (C.c_int32, [C.c_void_p]),
    "relp_robust_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_last_error": (C.c_char_p, [C.c_void_p]),
    "relp_version": (C.c_char_p, []),
    "relp_engine_create": (C.c_int, [C.POINTER(_MatrixData), C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "relp_engine_destroy": (None, [C.c_void_p]),
    "relp_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_select_primal_pivot_column": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_double)]),
    "relp_relative_costs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_generate_column": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "relp_generate_element": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "relp_select_primal_pivot_row": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "relp_select_primal_pivot_row_of": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "relp_bring_into_basis": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_int32)]),
    "relp_run": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "relp_run_dual": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "relp_select_dual_pivot_row": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "relp_select_dual_pivot_column": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "relp_set_right_hand_side": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_change_right_hand_side": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_set_upper_bound": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "relp_get_right_hand_side": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_rhs_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_change_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_set_cost": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_get_cost": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_cost_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_add_cuts": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_reserve_cuts": (C.c_int, [C.c_void_p, C.c_int32]),
    "relp_cut_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_add_columns": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_reserve_columns": (C.c_int, [C.c_void_p, C.c_int32]),
    "relp_column_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_remove_cuts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_remove_columns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_removal_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_row_ratios": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_rhs_ranging": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_ranging_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_gomory_cuts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "relp_gomory_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_trial_begin": (C.c_int, [C.c_void_p]),
    "relp_trial_end": (C.c_int, [C.c_void_p, C.c_int32]),
    "relp_trial_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_strong_branch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "relp_pool_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "relp_pool_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_pool_set_active": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "relp_pool_reduced_costs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_pool_price": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "relp_pool_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_pool_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_cutpool_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "relp_cutpool_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_cutpool_set_active": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "relp_cutpool_slacks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_cutpool_separate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int32)]),
    "relp_cutpool_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_cutpool_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_solve_relaxation": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "relp_from_basis": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_flush": (C.c_int, [C.c_void_p]),
    "relp_update_block": (C.c_int32, [C.c_void_p]),
    "relp_tab_load_batch": (C.c_int32, [C.c_void_p]),
    "relp_tab_column_rows": (C.c_int32, [C.c_void_p]),
    "relp_tab_column_rows_for": (C.c_int32, [C.c_int32, C.c_int32]),
    "relp_tab_flush_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_retab_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_lu_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_lu_lookahead_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_lu_kernel_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "relp_lu_set_device_factorisation": (C.c_int, [C.c_void_p, C.c_int32]),
    "relp_lu_device_factorisation_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_lu_factor_residual": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "relp_lu_phase_cycles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_basis_inverse_row": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "relp_should_refactor": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "relp_generate_column_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "relp_cost_difference_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    "relp_lu_change_basis": (C.c_int, [C.c_void_p, C.c_int32]),
    "relp_lu_set_factors": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "relp_lu_updates": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "relp_lu_get_update": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "relp_lu_get_upper": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "relp_shard_flush_begin": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "relp_shard_flush_end": (C.c_int, [C.c_void_p]),
    "relp_nr_rows": (C.c_int32, [C.c_void_p]),
    "relp_nr_columns": (C.c_int32, [C.c_void_p]),
    "relp_phase": (C.c_int32, [C.c_void_p]),
    "relp_nr_artificial": (C.c_int32, [C.c_void_p]),
    "relp_get_objective": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "relp_get_b": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_get_minus_pi": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_get_basis_indices": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_get_basis_inverse": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_current_bfs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "relp_get_iterations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_get_degenerate_pivots": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "relp_get_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.POINTER(C.c_int64)]),
    "relp_check_basis": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "relp_profile_enable": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32]),
    "relp_profile_read": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "relp_synth_fill_dense": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_void_p]),
    "relp_device_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64]),
    "relp_device_free": (C.c_int, [C.c_void_p]),
    "relp_shard_ranges": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int32)] * 5),
    "relp_shard_column_range": (None, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "relp_shard_candidate_len": (C.c_int64, [C.c_void_p]),
    "relp_shard_rho_len": (C.c_int64, [C.c_void_p]),
    "relp_shard_price": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_shard_select_column": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "relp_shard_ftran": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_shard_ratio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "relp_shard_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "relp_poll": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "relp_shard_pivot": (C.c_int, [C.c_void_p]),
    "relp_set_reinversion_interval": (C.c_int, [C.c_void_p, C.c_int64]),
    "relp_reinversions": (C.c_int64, [C.c_void_p]),
    "relp_shard_set_collectives": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "relp_shard_run": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "relp_shard_inject_failure": (C.c_int, [C.c_void_p, C.c_int64]),
    "relp_rccl_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "relp_rccl_attach": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "relp_shard_plan": (C.c_int, [C.POINTER(_MatrixData), C.POINTER(Config), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

_lib = None


def load_library():
    """Load ``librelp_engine.so``; raises if it is missing (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RelpError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def default_config(**overrides) -> Config:
    cfg = Config()
    load_library().relp_default_config(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def robust_config(**overrides) -> Config:
    """relp_robust_config: the f64 safeguards (largest-pivot ratio rule, textbook artificial removal, pivot rescue, adaptive
    re-inversion) and RELP_ENGINE_AUTO -- no per-file knobs."""
    cfg = Config()
    load_library().relp_robust_config(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def shard_column_range(nr_normal: int, rank: int, count: int) -> Tuple[int, int]:
    lo, hi = C.c_int32(), C.c_int32()
    load_library().relp_shard_column_range(nr_normal, rank, count, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_plan(provider: MatrixData, config: Config) -> Tuple[int, int]:
    """Structural columns [lo, hi) the rank ``config.shard_rank`` must supply (relp_shard_plan)."""
    md = _MatrixData()
    md.nr_normal, md.nr_eq, md.nr_range = provider.nr_normal, provider.nr_eq, provider.nr_range
    md.nr_le, md.nr_ge = provider.nr_le, provider.nr_ge
    ub = np.ascontiguousarray(provider.upper_bound, dtype=np.float64)
    md.upper_bound = ub.ctypes.data
    lo, hi = C.c_int32(), C.c_int32()
    st = load_library().relp_shard_plan(C.byref(md), C.byref(config), C.byref(lo), C.byref(hi))
    if st != 0:
        raise RelpError(f"relp_shard_plan failed ({st})")
    return lo.value, hi.value


class Tableau:
    """Device-resident ``Tableau<Carry<f64, BasisInverseRows<f64>>, K>`` (tableau/mod.rs:24-38)."""

    def __init__(self, provider: MatrixData, config: Optional[Config] = None, *, device_dense_ptr: Optional[int] = None,
                 device_dense_ld: Optional[int] = None, **config_overrides):
        """``Tableau::<_, Partially<_>>::new(provider)`` (kind/artificial/partially.rs:125).

        ``device_dense_ptr``: address of a column-major dense matrix already in HBM (e.g. a torch
        tensor's ``data_ptr()``), holding this shard's structural columns.
        """
        self._lib = load_library()
        cfg = config if config is not None else default_config()
        for k, v in config_overrides.items():
            setattr(cfg, k, v)
        self.config = cfg
        keep = []

        def ptr(a, dtype):
            arr = np.ascontiguousarray(a, dtype=dtype)
            keep.append(arr)
            return arr.ctypes.data

        md = _MatrixData()
        md.nr_normal, md.nr_eq, md.nr_range = provider.nr_normal, provider.nr_eq, provider.nr_range
        md.nr_le, md.nr_ge = provider.nr_le, provider.nr_ge
        if device_dense_ptr is not None:
            md.format, md.matrix_memory = FORMAT_DENSE, MEM_DEVICE
            md.dense = device_dense_ptr
            md.dense_ld = device_dense_ld or provider.nr_constraints
        elif provider.dense is not None:
            md.format, md.matrix_memory = FORMAT_DENSE, MEM_HOST
            dense = np.asfortranarray(provider.dense, dtype=np.float64)
            keep.append(dense)
            md.dense = dense.ctypes.data
            md.dense_ld = dense.shape[0]
        else:
            md.format, md.matrix_memory = FORMAT_CSC, MEM_HOST
            md.col_ptr = ptr(provider.col_ptr, np.int64)
            md.row_idx = ptr(provider.row_idx, np.int32)
            md.values = ptr(provider.values, np.float64)
        md.b = ptr(provider.b, np.float64)
        md.ranges = ptr(provider.ranges, np.float64)
        md.cost = ptr(provider.cost, np.float64)
        md.upper_bound = ptr(provider.upper_bound, np.float64)
        h = C.c_void_p()
        st = self._lib.relp_engine_create(C.byref(md), C.byref(cfg), C.byref(h))
        self._h = h
        if st != 0:
            msg = self._lib.relp_last_error(h).decode() if h else "allocation failed"
            if h:
                self._lib.relp_engine_destroy(h)
            self._h = None
            raise RelpError(f"relp_engine_create failed ({st}): {msg}")
        self.provider = provider
        del keep

    # -- plumbing ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.relp_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise RelpError(f"relp call failed ({st}): {self._lib.relp_last_error(self._h).decode()}")

    @property
    def handle(self):
        return self._h

    def set_stream(self, hip_stream: int):
        self._ck(self._lib.relp_set_stream(self._h, hip_stream))

    # -- sizes / kind -----------------------------------------------------------------------
    def nr_rows(self) -> int:
        return self._lib.relp_nr_rows(self._h)

    def nr_columns(self) -> int:
        return self._lib.relp_nr_columns(self._h)

    def nr_artificial_variables(self) -> int:
        return self._lib.relp_nr_artificial(self._h)

    @property
    def phase(self) -> int:
        return self._lib.relp_phase(self._h)

    # -- one pivot (tableau/mod.rs:47-247, pivot_rule.rs:25) ---------------------------------
    def select_primal_pivot_column(self, rule: int) -> Optional[Tuple[int, float]]:
        found, col, cost = C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self._lib.relp_select_primal_pivot_column(self._h, rule, C.byref(found), C.byref(col), C.byref(cost)))
        return (col.value, cost.value) if found.value else None

    def relative_costs(self) -> np.ndarray:
        out = np.zeros(self.nr_columns())
        self._ck(self._lib.relp_relative_costs(self._h, out.ctypes.data))
        return out

    def relative_cost(self, j: int) -> float:
        return float(self.relative_costs()[j])

    def generate_column(self, j: int) -> np.ndarray:
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_generate_column(self._h, j, out.ctypes.data))
        return out

    def generate_element(self, i: int, j: int) -> float:
        v = C.c_double()
        self._ck(self._lib.relp_generate_element(self._h, i, j, C.byref(v)))
        return v.value

    def set_reinversion_interval(self, pivots: int) -> None:
        """Revised and tableau engines (unsharded), any number of rows: rebuild B^-1 (revised) or the tableau B^-1 [A | I]
        (tableau), b, -pi / the reduced costs and the objective from the columns of the current basis every `pivots` basis
        changes (0 = never)."""
        self._ck(self._lib.relp_set_reinversion_interval(self._h, int(pivots)))

    def reinversions(self) -> int:
        return int(self._lib.relp_reinversions(self._h))

    def select_primal_pivot_row(self, column=None) -> Optional[int]:
        """tableau/mod.rs:221-247.  Without an argument: on the last generated column (device resident);
        with a dense column of m entries: the reference's signature."""
        found, row = C.c_int32(), C.c_int32()
        if column is None:
            self._ck(self._lib.relp_select_primal_pivot_row(self._h, C.byref(found), C.byref(row)))
        else:
            col = np.ascontiguousarray(column, dtype=np.float64)
            if col.shape != (self.nr_rows(),):
                raise ValueError("column must have nr_rows() entries")
            self._ck(self._lib.relp_select_primal_pivot_row_of(self._h, col.ctypes.data_as(C.POINTER(C.c_double)),
                                                              C.byref(found), C.byref(row)))
        return row.value if found.value else None

    def bring_into_basis(self, column: int, row: int, cost: float) -> int:
        leaving = C.c_int32()
        self._ck(self._lib.relp_bring_into_basis(self._h, column, row, cost, C.byref(leaving)))
        return leaving.value

    # -- loops ------------------------------------------------------------------------------
    def run(self, max_iters: int) -> Tuple[int, int]:
        """Up to ``max_iters`` basis changes of the current phase; returns (iterations, outcome)."""
        done, oc = C.c_int64(), C.c_int32()
        self._ck(self._lib.relp_run(self._h, max_iters, C.byref(done), C.byref(oc)))
        return done.value, oc.value

    # -- dual simplex (tableau engine, phase 2; beyond the reference) ---------------------------
    def run_dual(self, max_iters: int) -> Tuple[int, int]:
        """Up to ``max_iters`` dual pivots from a dual feasible basis; returns (iterations, outcome) with outcome OPTIMAL,
        INFEASIBLE or RUNNING (relp_run_dual)."""
        done, oc = C.c_int64(), C.c_int32()
        self._ck(self._lib.relp_run_dual(self._h, max_iters, C.byref(done), C.byref(oc)))
        return done.value, oc.value

    def select_dual_pivot_row(self) -> Optional[int]:
        """The leaving row of a dual pivot: the most negative b_i; None when no row is infeasible."""
        found, row = C.c_int32(), C.c_int32()
        self._ck(self._lib.relp_select_dual_pivot_row(self._h, C.byref(found), C.byref(row)))
        return row.value if found.value else None

    def select_dual_pivot_column(self, row: int) -> Optional[int]:
        """The entering column of a dual pivot in tableau row ``row``; None when the row has no candidate."""
        found, col = C.c_int32(), C.c_int32()
        self._ck(self._lib.relp_select_dual_pivot_column(self._h, int(row), C.byref(found), C.byref(col)))
        return col.value if found.value else None

    def set_right_hand_side(self, rhs) -> None:
        """A new right-hand side (nr_rows() entries in the engine's row order, any sign) for the current basis: the tableau is
        re-tabulated, ``run_dual`` re-solves from there."""
        arr = np.ascontiguousarray(rhs, dtype=np.float64)
        if arr.shape != (self.nr_rows(),):
            raise ValueError("rhs must have nr_rows() entries")
        self._ck(self._lib.relp_set_right_hand_side(self._h, arr.ctypes.data))

    def change_right_hand_side(self, rows, values) -> None:
        """rhs[rows[k]] = values[k] on the current basis without a re-tabulation (relp_change_right_hand_side): b moves by the
        changed rows' columns of B^-1, read off the tableau; the reduced costs, the basis and the open update block stay.  ``rows``
        are engine rows in the current order, each named once; ``run_dual`` re-solves from there."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if r.ndim != 1 or r.shape != v.shape:
            raise ValueError("rows and values must be one-dimensional and of the same length")
        self._ck(self._lib.relp_change_right_hand_side(self._h, r.ctypes.data, v.ctypes.data, r.shape[0]))

    def set_upper_bound(self, column: int, value: float) -> None:
        """The upper bound of structural column ``column`` (finite at create) becomes ``value``: the in-place change of its bound
        row (relp_set_upper_bound)."""
        self._ck(self._lib.relp_set_upper_bound(self._h, int(column), float(value)))

    def right_hand_side(self) -> np.ndarray:
        """The rhs in effect, nr_rows() entries in the engine's row order (relp_get_right_hand_side)."""
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_get_right_hand_side(self._h, out.ctypes.data))
        return out

    def rhs_stats(self) -> Tuple[int, int, int, int]:
        """(in-place rhs changes so far, columns of B^-1 they read, pending rows of the update block at the last change, shares of
        the list in its last launch); relp_rhs_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_rhs_stats(self._h, out))
        return tuple(int(x) for x in out)

    def change_cost(self, columns, values) -> None:
        """cost[columns[k]] = values[k] on the current basis without a flush or a re-tabulation (relp_change_cost): the reduced
        costs move by the tableau rows of the changed basic columns, read off T0 + W R0; b, the basis and the open update block
        stay.  ``columns`` are structural columns, each named once; ``run`` re-solves from there."""
        c = np.ascontiguousarray(columns, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if c.ndim != 1 or c.shape != v.shape:
            raise ValueError("columns and values must be one-dimensional and of the same length")
        self._ck(self._lib.relp_change_cost(self._h, c.ctypes.data, v.ctypes.data, c.shape[0]))

    def set_cost(self, cost) -> None:
        """Every structural cost at once (relp_set_cost): an open update block is flushed, then d = c - c_B' T0 in one pass over
        the tableau.  No re-tabulation; the call to make when most costs move."""
        arr = np.ascontiguousarray(cost, dtype=np.float64)
        if arr.shape != (self.provider.nr_normal,):
            raise ValueError("cost must have one entry per structural column")
        self._ck(self._lib.relp_set_cost(self._h, arr.ctypes.data))

    def cost(self) -> np.ndarray:
        """The structural costs in effect, one per structural column (relp_get_cost)."""
        out = np.zeros(self.provider.nr_normal)
        self._ck(self._lib.relp_get_cost(self._h, out.ctypes.data))
        return out

    def cost_stats(self) -> Tuple[int, int, int, int]:
        """(in-place cost changes so far, tableau rows they read, pending rows of the update block at the last change, shares of
        the basic list in its last launch); relp_cost_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_cost_stats(self._h, out))
        return tuple(int(x) for x in out)

    def add_cuts(self, G, rhs) -> None:
        """The cuts ``G x <= rhs`` over the structural columns become rows behind every existing row, on the current basis and
        without a flush or a re-tabulation (relp_add_cuts); cut k is row ``nr_rows() + k`` and its slack, basic in that row,
        column ``nr_columns() + k`` (both read before the call).  ``G`` is a dense ``count x nr_normal`` array or a CSR triple
        ``(row_ptr, col_idx, values)``; ``run_dual`` re-solves from there."""
        count, ptr, idx, val, beta = self._csr_cuts(G, rhs)
        self._ck(self._lib.relp_add_cuts(self._h, count, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, beta.ctypes.data))

    def _csr_cuts(self, G, rhs):
        """(count, row_ptr, col_idx, values, rhs) of cuts given as a dense ``count x nr_normal`` array or a CSR triple: what
        relp_add_cuts and relp_cutpool_create take."""
        n = self.provider.nr_normal
        if isinstance(G, tuple):
            if len(G) != 3:
                raise ValueError("a CSR triple is (row_ptr, col_idx, values)")
            ptr = np.ascontiguousarray(G[0], dtype=np.int64)
            idx = np.ascontiguousarray(G[1], dtype=np.int32)
            val = np.ascontiguousarray(G[2], dtype=np.float64)
            if ptr.ndim != 1 or ptr.shape[0] < 1 or idx.ndim != 1 or idx.shape != val.shape:
                raise ValueError("row_ptr, col_idx and values must be one-dimensional, the latter two of the same length")
            if ptr.shape[0] > 1 and ptr[-1] > idx.shape[0]:
                raise ValueError("row_ptr reaches beyond col_idx")
        else:
            dense = np.atleast_2d(np.asarray(G, dtype=np.float64))
            if dense.ndim != 2 or dense.shape[1] != n:
                raise ValueError("G must have one column per structural column")
            rows, cols = np.nonzero(dense)             # row-major: ascending row, then column
            ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=dense.shape[0])))).astype(np.int64)
            idx = np.ascontiguousarray(cols, dtype=np.int32)
            val = np.ascontiguousarray(dense[rows, cols], dtype=np.float64)
        count = ptr.shape[0] - 1
        beta = np.ascontiguousarray(np.atleast_1d(rhs), dtype=np.float64)
        if beta.shape != (count,):
            raise ValueError("rhs must have one entry per cut")
        return count, ptr, idx, val, beta

    def cut_pool(self, G, rhs) -> "CutPool":
        """A pool of candidate cuts ``G x <= rhs`` kept on the device (relp_cutpool_create): ``G`` and ``rhs`` as ``add_cuts`` takes
        them.  The pool is separated against the vertex as it stands (``CutPool.separate``) and its winners are added in place
        (``CutPool.add``) without their coefficients going through the host again; it belongs to this tableau."""
        count, ptr, idx, val, beta = self._csr_cuts(G, rhs)
        handle = C.c_void_p()
        self._ck(self._lib.relp_cutpool_create(self._h, count, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, beta.ctypes.data,
                                               C.byref(handle)))
        return CutPool(self, handle, count)

    def reserve_cuts(self, rows: int) -> None:
        """Room for ``rows`` cut rows in all, without adding any (relp_reserve_cuts): the tableau is re-allocated and copied
        once, here, instead of inside an ``add_cuts``."""
        self._ck(self._lib.relp_reserve_cuts(self._h, int(rows)))

    def cut_stats(self) -> Tuple[int, int, int, int]:
        """(cuts in the tableau, cut rows there is room for, tableau rows the last add_cuts read, pending rows of the update block
        at that call); relp_cut_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_cut_stats(self._h, out))
        return tuple(int(x) for x in out)

    def add_columns(self, A_new, cost) -> None:
        """New variables ``x >= 0`` with the columns ``A_new`` over the engine rows and the costs ``cost`` become columns behind
        every existing column, non-basic, on the current basis and without a flush or a re-tabulation (relp_add_columns); column k
        is column ``nr_columns() + k`` (read before the call).  ``A_new`` is a dense ``nr_rows() x count`` array, one vector with a
        scalar cost, or a CSC triple ``(col_ptr, row_idx, values)``; ``run`` re-solves from there."""
        count, ptr, idx, val, c = self._csc_columns(A_new, cost)
        self._ck(self._lib.relp_add_columns(self._h, count, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, c.ctypes.data))

    def _csc_columns(self, A_new, cost):
        """(count, col_ptr, row_idx, values, cost) of columns given as a dense ``nr_rows() x count`` array, one vector with a scalar
        cost, or a CSC triple: what relp_add_columns and relp_pool_create take."""
        if isinstance(A_new, tuple):
            if len(A_new) != 3:
                raise ValueError("a CSC triple is (col_ptr, row_idx, values)")
            ptr = np.ascontiguousarray(A_new[0], dtype=np.int64)
            idx = np.ascontiguousarray(A_new[1], dtype=np.int32)
            val = np.ascontiguousarray(A_new[2], dtype=np.float64)
            if ptr.ndim != 1 or ptr.shape[0] < 1 or idx.ndim != 1 or idx.shape != val.shape:
                raise ValueError("col_ptr, row_idx and values must be one-dimensional, the latter two of the same length")
            if ptr.shape[0] > 1 and ptr[-1] > idx.shape[0]:
                raise ValueError("col_ptr reaches beyond row_idx")
        else:
            dense = np.asarray(A_new, dtype=np.float64)
            if dense.ndim == 1:
                dense = dense.reshape(-1, 1)
            if dense.ndim != 2 or dense.shape[0] != self.nr_rows():
                raise ValueError("A_new must have one row per engine row")
            cols, rows = np.nonzero(dense.T)           # column-major: ascending column, then row
            ptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=dense.shape[1])))).astype(np.int64)
            idx = np.ascontiguousarray(rows, dtype=np.int32)
            val = np.ascontiguousarray(dense[rows, cols], dtype=np.float64)
        count = ptr.shape[0] - 1
        c = np.ascontiguousarray(np.atleast_1d(cost), dtype=np.float64)
        if c.shape != (count,):
            raise ValueError("cost must have one entry per column")
        return count, ptr, idx, val, c

    def pool(self, A, cost) -> "ColumnPool":
        """A pool of candidate columns ``x >= 0`` kept on the device (relp_pool_create): ``A`` and ``cost`` as ``add_columns`` takes
        them.  The pool is priced against the duals as they stand (``ColumnPool.price``) and its winners are added in place
        (``ColumnPool.add``) without their coefficients going through the host again; it belongs to this tableau."""
        count, ptr, idx, val, c = self._csc_columns(A, cost)
        handle = C.c_void_p()
        self._ck(self._lib.relp_pool_create(self._h, count, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, c.ctypes.data, C.byref(handle)))
        return ColumnPool(self, handle, count)

    def reserve_columns(self, columns: int) -> None:
        """Room for ``columns`` added columns in all, without adding any (relp_reserve_columns): the tableau is re-allocated and
        copied once, here, instead of inside an ``add_columns``."""
        self._ck(self._lib.relp_reserve_columns(self._h, int(columns)))

    def column_stats(self) -> Tuple[int, int, int, int]:
        """(added columns in the tableau, columns there is room for, identity columns the last add_columns read, pending rows of
        the update block at that call); relp_column_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_column_stats(self._h, out))
        return tuple(int(x) for x in out)

    def remove_cuts(self, rows) -> None:
        """The cut rows ``rows`` (engine row indices, each once, any order) leave the tableau in place, each with its slack, which
        must be basic -- in whichever tableau row (relp_remove_cuts).  The open update block is flushed first; surviving rows and
        columns close up in order and keep their bits; the room stays for the next ``add_cuts``."""
        r = np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        self._ck(self._lib.relp_remove_cuts(self._h, r.ctypes.data, r.shape[0]))

    def remove_columns(self, columns) -> None:
        """The added columns ``columns`` (provider column indices of columns from ``add_columns``, each once, any order, each
        non-basic) leave the tableau in place (relp_remove_columns); the columns behind them close up in order."""
        c = np.ascontiguousarray(np.atleast_1d(columns), dtype=np.int32)
        if c.ndim != 1:
            raise ValueError("columns must be one-dimensional")
        self._ck(self._lib.relp_remove_columns(self._h, c.ctypes.data, c.shape[0]))

    def removal_stats(self) -> Tuple[int, int, int, int]:
        """(cuts removed so far, added columns removed so far, tableau entries the last removal moved, pending rows of the update
        block it flushed); relp_removal_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_removal_stats(self._h, out))
        return tuple(int(x) for x in out)

    def _ratio_query(self, call, rows):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        n = r.shape[0]
        ratio0, ratio1 = np.full(n, np.inf), np.full(n, np.inf)
        index0, index1 = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        self._ck(call(self._h, r.ctypes.data, n, ratio0.ctypes.data, index0.ctypes.data, ratio1.ctypes.data, index1.ctypes.data))
        return ratio0, index0, ratio1, index1

    def row_ratios(self, rows):
        """(down_ratio, down_column, up_ratio, up_column), one entry per listed engine row (relp_row_ratios): the minimum of
        d_j / -T[r,j] over the non-basic columns with T[r,j] < -tol_pivot (down) and of d_j / T[r,j] over T[r,j] > tol_pivot
        (up), with the lowest column inside the tie band; (inf, -1) without a candidate.  down is the entering rule of
        ``select_dual_pivot_column(r)``.  Read as the penalty per unit the row's basic variable is pushed down / up, or as the
        range [c - down, c + up] of its cost.  Read-only; any order, repeats allowed."""
        return self._ratio_query(self._lib.relp_row_ratios, rows)

    def rhs_ranging(self, rows):
        """(decrease, decrease_row, increase, increase_row), one entry per listed engine row (relp_rhs_ranging): the basis stays
        primal feasible while rhs[row] stays within [rhs - decrease, rhs + increase]; ``*_row`` is the row that blocks, (inf, -1)
        when nothing does.  Read-only."""
        return self._ratio_query(self._lib.relp_rhs_ranging, rows)

    def ranging_stats(self) -> Tuple[int, int, int, int]:
        """(row_ratios calls so far, rows they covered, rhs_ranging calls so far, pending rows of the update block at the last
        call of either); relp_ranging_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_ranging_stats(self._h, out))
        return tuple(int(x) for x in out)

    def gomory_cuts(self, rows, is_integer=None, kind=GOMORY_FRACTIONAL, away=1e-6):
        """(G, rhs, fraction, status), one entry per listed engine row (relp_gomory_cuts): the Gomory cut ``G[k] x <= rhs[k]`` of
        tableau row ``rows[k]`` over the structural columns, in the form ``add_cuts`` takes, violated by the current vertex by
        ``fraction[k] = b_r - floor(b_r)``.  ``is_integer``: one flag per provider column (``nr_columns()``), None = all integer;
        ``kind`` GOMORY_FRACTIONAL or GOMORY_MIXED.  ``status[k]``: GOMORY_CUT (0) a cut was made, else the entry is skipped (all
        zero): GOMORY_NOT_INTEGER (the basic column is not flagged), GOMORY_FRACTION (the fraction is within ``away`` of 0 or
        1), GOMORY_ARTIFICIAL, GOMORY_CONTINUOUS (a continuous column in a fractional cut).  Read-only; any order, repeats
        allowed."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        flags = None
        if is_integer is not None:
            flags = np.ascontiguousarray(np.asarray(is_integer) != 0, dtype=np.uint8)
            if flags.shape != (self.nr_columns(),):
                raise ValueError("is_integer must have one flag per provider column")
        n = r.shape[0]
        G, rhs = np.zeros((n, self.provider.nr_normal)), np.zeros(n)
        fraction, status = np.zeros(n), np.full(n, -1, dtype=np.int32)
        self._ck(self._lib.relp_gomory_cuts(self._h, r.ctypes.data, n, None if flags is None else flags.ctypes.data, int(kind),
                                            float(away), G.ctypes.data, rhs.ctypes.data, fraction.ctypes.data, status.ctypes.data))
        return G, rhs, fraction, status

    def gomory_stats(self) -> Tuple[int, int, int, int]:
        """(gomory_cuts calls so far, list entries they covered, cuts made, pending rows of the update block at the last call);
        relp_gomory_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_gomory_stats(self._h, out))
        return tuple(int(x) for x in out)

    # -- trials (tableau engine, phase 2; beyond the reference) ---------------------------------
    def trial_begin(self) -> None:
        """Opens a trial (relp_trial_begin): what ``change_right_hand_side``, ``set_upper_bound``, ``change_cost``, ``add_cuts``
        within the reserved room and ``run_dual`` can change is saved -- no flush, no copy of the tableau -- and ``trial_end()``
        puts it back to the bit.  Inside a trial ``run_dual`` pivots only while the update block has room and never flushes or
        re-inverts; whatever flushes, rebuilds, re-allocates or compacts is refused.  Trials do not nest."""
        self._ck(self._lib.relp_trial_begin(self._h))

    def trial_end(self, keep: bool = False) -> None:
        """Ends the open trial (relp_trial_end): ``keep=False`` restores every getter and every ``*_stats`` to the bit,
        ``keep=True`` drops the snapshot and leaves the state as it is."""
        self._ck(self._lib.relp_trial_end(self._h, 1 if keep else 0))

    def trial_stats(self) -> Tuple[int, int, int, int]:
        """(trials begun, trials rolled back, bytes the last snapshot held, pivots the last trial could still have made when it
        ended); relp_trial_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_trial_stats(self._h, out))
        return tuple(int(x) for x in out)

    def trial(self) -> "Trial":
        """``with t.trial() as scope: ...``: a trial that is rolled back on exit unless ``scope.keep()`` was called."""
        return Trial(self)

    def strong_branch(self, rows, max_pivots: int, away: float = 1e-6):
        """(objective, outcome, pivots, status) of relp_strong_branch: per listed engine row r with a fractional structural basic
        column x_j, ``objective[k]`` / ``outcome[k]`` / ``pivots[k]`` hold (down, up): the child LPs x_j <= floor(b_r) and
        x_j >= ceil(b_r) after at most ``max_pivots`` dual pivots each, rolled back afterwards.  outcome OPTIMAL, INFEASIBLE
        (objective inf) or RUNNING (the objective is still a valid bound: the dual objective is monotone).  ``status[k]``:
        BRANCH_EVALUATED, BRANCH_NOT_STRUCTURAL or BRANCH_FRACTION (skipped: nan, -1, 0).  May grow the room for one cut and
        flush the open block once before the first trial; read-only otherwise."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        n = r.shape[0]
        objective, outcome = np.full((n, 2), np.nan), np.full((n, 2), -1, dtype=np.int32)
        pivots, status = np.zeros((n, 2), dtype=np.int32), np.full(n, -1, dtype=np.int32)
        self._ck(self._lib.relp_strong_branch(self._h, r.ctypes.data, n, int(max_pivots), float(away), objective.ctypes.data,
                                              outcome.ctypes.data, pivots.ctypes.data, status.ctypes.data))
        return objective, outcome, pivots, status

    def cost_ranging(self, columns):
        """(decrease, increase) per structural column j of ``columns``: the basis stays optimal while c_j stays within
        [c_j - decrease, c_j + increase].  A non-basic column gives (d_j, inf); a basic one the (down, up) of ``row_ratios`` on
        its row.  Built on relative_costs(), basis_indices() and row_ratios()."""
        cols = np.ascontiguousarray(columns, dtype=np.int64)
        if cols.ndim != 1:
            raise ValueError("columns must be one-dimensional")
        basis = self.basis_indices()
        row_of = {int(c): i for i, c in enumerate(basis)}
        d = np.asarray(self.relative_costs())
        dec, inc = np.empty(cols.shape[0]), np.full(cols.shape[0], np.inf)
        basic = [k for k, j in enumerate(cols) if int(j) in row_of]
        for k, j in enumerate(cols):
            if int(j) not in row_of:
                dec[k] = d[int(j)]
        if basic:
            down, _, up, _ = self.row_ratios([row_of[int(cols[k])] for k in basic])
            dec[basic], inc[basic] = down, up
        return dec, inc

    def solve_relaxation(self, max_iters: int = 1 << 40) -> int:
        oc = C.c_int32()
        self._ck(self._lib.relp_solve_relaxation(self._h, max_iters, C.byref(oc)))
        return oc.value

    def flush(self) -> None:
        """Fold pending deferred updates into the explicit inverse."""
        self._ck(self._lib.relp_flush(self._h))

    def update_block(self) -> int:
        return self._lib.relp_update_block(self._h)

    def load_batch(self) -> int:
        """Tableau engine: pending rows the per-pivot kernels load per round trip (RELP_TAB_LOAD_BATCH at create)."""
        return self._lib.relp_tab_load_batch(self._h)

    def column_rows(self) -> int:
        """Tableau engine: rows per workgroup of the column kernel in the fused loop (RELP_TAB_COLUMN_ROWS at create)."""
        return self._lib.relp_tab_column_rows(self._h)

    def flush_stats(self) -> Tuple[int, int]:
        """Tableau engine: (flushes, columns those flushes rewrote) since create."""
        out = (C.c_int64 * 2)()
        self._ck(self._lib.relp_tab_flush_stats(self._h, out))
        return int(out[0]), int(out[1])

    def retab_stats(self) -> Tuple[int, int, int, int]:
        """Revised and tableau engines: (batch solves of the rebuilds with the work vector in LDS, batch solves with it in
        global slabs, workgroups of the last launch of the second kind, bytes of the slab buffer); relp_retab_stats."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_retab_stats(self._h, out))
        return tuple(int(v) for v in out)

    def engine_kind(self) -> int:
        """The engine in use (RELP_ENGINE_AUTO resolved at create)."""
        return int(self._lib.relp_engine_kind(self._h))

    def robust_stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self._ck(self._lib.relp_robust_stats(self._h, out))
        return dict(zip(("small_pivots", "columns_barred", "confirmations", "reinversion_interval"), (int(v) for v in out)))

    def lu_stats(self) -> dict:
        """Factor statistics of the LU engine (relp_lu_stats)."""
        out = (C.c_int64 * 8)()
        self._ck(self._lib.relp_lu_stats(self._h, out))
        keys = ("refactorisations", "m", "nnz_l", "nnz_u", "levels_l", "levels_u", "levels_ut", "levels_lt")
        stats = dict(zip(keys, (int(v) for v in out)))
        la = (C.c_int64 * 4)()
        self._ck(self._lib.relp_lu_lookahead_stats(self._h, la))
        stats.update(lookahead_installs=int(la[0]), replayed_changes=int(la[1]), lookahead=int(la[2]), fuse_lanes=int(la[3]))
        return stats

    def lu_kernel_layout(self) -> dict:
        """How the LU engine's pivot loop runs (relp_lu_kernel_layout): persistent kernel or product-form fallback, the
        kernel's layout (0 all in LDS, 1 big, 2 nothing per row in LDS), dense-tail slots, grid PRICE."""
        out = (C.c_int32 * 4)()
        self._ck(self._lib.relp_lu_kernel_layout(self._h, out))
        return {"persistent_kernel": bool(out[0]), "layout": int(out[1]), "tail_slots": int(out[2]), "grid_price": bool(out[3])}

    def lu_set_device_factorisation(self, on: bool) -> None:
        """Refactorise on the device from now on (relp_lu_set_device_factorisation; LUDecomposition::invert)."""
        self._ck(self._lib.relp_lu_set_device_factorisation(self._h, 1 if on else 0))

    def lu_factor_residual(self) -> float:
        """max |P B Q - L U| for the factors in use (relp_lu_factor_residual)."""
        out = C.c_double()
        self._ck(self._lib.relp_lu_factor_residual(self._h, C.byref(out)))
        return out.value

    def lu_device_factorisation_stats(self) -> dict:
        out = (C.c_int64 * 6)()
        self._ck(self._lib.relp_lu_device_factorisation_stats(self._h, out))
        keys = ("enabled", "device_factorisations", "host_fallbacks", "kernel_us", "last_bump", "last_peeled")
        return dict(zip(keys, (int(v) for v in out)))

    # -- BasisInverse surface (carry/mod.rs:68-157) ---------------------------------------------
    def basis_inverse_row(self, row: int) -> np.ndarray:
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_basis_inverse_row(self._h, row, out.ctypes.data))
        return out

    def should_refactor(self) -> bool:
        v = C.c_int32()
        self._ck(self._lib.relp_should_refactor(self._h, C.byref(v)))
        return bool(v.value)

    @staticmethod
    def _sparse(column):
        idx = np.ascontiguousarray([i for i, _ in column], dtype=np.int32)
        val = np.ascontiguousarray([v for _, v in column], dtype=np.float64)
        return idx, val

    def generate_column_of(self, column) -> np.ndarray:
        """`BasisInverse::generate_column(original_column)` for sorted (row, value) pairs."""
        idx, val = self._sparse(column)
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_generate_column_of(self._h, idx.ctypes.data, val.ctypes.data, len(idx), out.ctypes.data))
        return out

    def cost_difference_of(self, column) -> float:
        idx, val = self._sparse(column)
        v = C.c_double()
        self._ck(self._lib.relp_cost_difference_of(self._h, idx.ctypes.data, val.ctypes.data, len(idx), C.byref(v)))
        return v.value

    def lu_change_basis(self, pivot_row_index: int) -> None:
        self._ck(self._lib.relp_lu_change_basis(self._h, pivot_row_index))

    def lu_set_factors(self, lower_columns, upper_columns) -> None:
        """`LUDecomposition { lower_triangular, upper_triangular, .. }` literally (P = Q = I): lists of columns of
        (row, value) pairs; L without its unit diagonal (m - 1 or m columns), U with its diagonal."""
        m = self.nr_rows()

        def csc(cols):
            cols = list(cols) + [[] for _ in range(m - len(cols))]
            ptr = np.zeros(m + 1, dtype=np.int64)
            for j, c in enumerate(cols):
                ptr[j + 1] = ptr[j] + len(c)
            idx = np.ascontiguousarray([i for c in cols for i, _ in c] or [0], dtype=np.int32)
            val = np.ascontiguousarray([v for c in cols for _, v in c] or [0.0], dtype=np.float64)
            return ptr, idx, val
        lp, li, lv = csc(lower_columns)
        up, ui, uv = csc(upper_columns)
        self._ck(self._lib.relp_lu_set_factors(self._h, lp.ctypes.data, li.ctypes.data, lv.ctypes.data, up.ctypes.data,
                                               ui.ctypes.data, uv.ctypes.data))

    def lu_updates(self):
        """[(pivot, [(position, value), ...]), ...]: the reference's `updates` (EtaFile values + RotateToBack index)."""
        n = C.c_int32()
        self._ck(self._lib.relp_lu_updates(self._h, C.byref(n)))
        m = self.nr_rows()
        out = []
        for k in range(n.value):
            pivot, nnz = C.c_int32(), C.c_int32()
            idx, val = np.zeros(m, dtype=np.int32), np.zeros(m)
            self._ck(self._lib.relp_lu_get_update(self._h, k, C.byref(pivot), idx.ctypes.data, val.ctypes.data, m, C.byref(nnz)))
            out.append((pivot.value, list(zip(idx[:nnz.value].tolist(), val[:nnz.value].tolist()))))
        return out

    def lu_upper(self):
        """The reference's `upper_triangular`: list of columns of (row, value), diagonal last."""
        m = self.nr_rows()
        cap = m * (m + 1) // 2 + m
        ptr, idx, val, nnz = np.zeros(m + 1, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(cap), C.c_int64()
        self._ck(self._lib.relp_lu_get_upper(self._h, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, cap, C.byref(nnz)))
        return [list(zip(idx[ptr[j]:ptr[j + 1]].tolist(), val[ptr[j]:ptr[j + 1]].tolist())) for j in range(m)]

    PHASE_NAMES = ("price", "scatter", "l_solve", "eta_forward", "spike_push", "u_solve", "ratio", "b_update", "u_bar",
                   "ut_solve", "compact", "eta_backward", "lt_solve", "vectors", "load_store", "stage_and_level0")

    def lu_phase_cycles(self) -> dict:
        out = (C.c_int64 * 16)()
        self._ck(self._lib.relp_lu_phase_cycles(self._h, out))
        return dict(zip(self.PHASE_NAMES, (int(v) for v in out)))

    def from_basis(self, basis_columns) -> None:
        arr = np.ascontiguousarray(basis_columns, dtype=np.int32)
        self._ck(self._lib.relp_from_basis(self._h, arr.ctypes.data))

    # -- state ------------------------------------------------------------------------------
    def objective_function_value(self) -> float:
        v = C.c_double()
        self._ck(self._lib.relp_get_objective(self._h, C.byref(v)))
        return v.value

    def b(self) -> np.ndarray:
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_get_b(self._h, out.ctypes.data))
        return out

    def minus_pi(self) -> np.ndarray:
        out = np.zeros(self.nr_rows())
        self._ck(self._lib.relp_get_minus_pi(self._h, out.ctypes.data))
        return out

    def basis_indices(self) -> np.ndarray:
        out = np.zeros(self.nr_rows(), dtype=np.int32)
        self._ck(self._lib.relp_get_basis_indices(self._h, out.ctypes.data))
        return out

    def basis_inverse(self) -> np.ndarray:
        m = self.nr_rows()
        out = np.zeros((m, m))
        self._ck(self._lib.relp_get_basis_inverse(self._h, out.ctypes.data))
        return out

    def current_bfs(self) -> List[Tuple[int, float]]:
        m = self.nr_rows()
        cols, vals, cnt = np.zeros(m, dtype=np.int32), np.zeros(m), C.c_int32()
        self._ck(self._lib.relp_current_bfs(self._h, cols.ctypes.data, vals.ctypes.data, m, C.byref(cnt)))
        return list(zip(cols[:cnt.value].tolist(), vals[:cnt.value].tolist()))

    def degenerate_pivots(self) -> int:
        """Pivots so far with ratio exactly 0 (the basis changed, b did not)."""
        out = C.c_int64()
        self._ck(self._lib.relp_get_degenerate_pivots(self._h, C.byref(out)))
        return out.value

    def iterations(self) -> int:
        v = C.c_int64()
        self._ck(self._lib.relp_get_iterations(self._h, C.byref(v)))
        return v.value

    def trace(self) -> List[Tuple[int, int, int, int]]:
        cap = int(self.config.trace_capacity)
        arrs = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(4)]
        cnt = C.c_int64()
        self._ck(self._lib.relp_get_trace(self._h, *[a.ctypes.data for a in arrs], cap, C.byref(cnt)))
        k = min(cnt.value, cap)
        return list(zip(*(a[:k].tolist() for a in arrs)))

    def check_basis(self) -> Tuple[float, float, float]:
        """``is_in_basic_feasible_solution_state`` (tableau/mod.rs:253-289) as three residuals."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._ck(self._lib.relp_check_basis(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- profiling --------------------------------------------------------------------------
    def profile_enable(self, enable: bool, max_launches: int = 0, sample_every: int = 1):
        self._ck(self._lib.relp_profile_enable(self._h, int(enable), max_launches, sample_every))

    def profile_read(self):
        out = {}
        for kid, name in enumerate(KERNEL_NAMES):
            n, ms = C.c_int64(), C.c_double()
            self._ck(self._lib.relp_profile_read(self._h, kid, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out


def phase_one_primal(tableau: Tableau, max_iters: int = 1 << 40) -> int:
    """phase_one::primal (phase_one.rs:125-170)."""
    if tableau.phase != 1:
        raise RelpError("tableau is not artificial")
    return tableau.run(max_iters)[1]


def phase_two_primal(tableau: Tableau, max_iters: int = 1 << 40) -> int:
    """phase_two::primal (phase_two.rs:22-51)."""
    if tableau.phase != 2:
        raise RelpError("tableau still has artificial variables")
    return tableau.run(max_iters)[1]


def phase_two_dual(tableau: Tableau, max_iters: int = 1 << 40) -> int:
    """The dual simplex loop from a dual feasible basis (relp_run_dual; the reference has none)."""
    if tableau.phase != 2:
        raise RelpError("tableau still has artificial variables")
    return tableau.run_dual(max_iters)[1]


class Trial:
    """The scope of ``Tableau.trial()``: begins a trial on entry and ends it on exit, rolled back unless ``keep()`` was called."""

    def __init__(self, tableau: Tableau):
        self._t, self._keep = tableau, False

    def keep(self) -> None:
        self._keep = True

    def __enter__(self) -> "Trial":
        self._t.trial_begin()
        return self

    def __exit__(self, *exc) -> bool:
        self._t.trial_end(self._keep)
        return False


class _DevicePool:
    """What ``ColumnPool`` and ``CutPool`` share: the handle, the open/closed checks and the calls that differ in their C name alone
    (``_PREFIX`` + ``_destroy`` / ``_add`` / ``_set_active`` / ``_stats``); the two classes keep ``add``, ``set_active`` and ``stats``
    as one-line methods with their own docstrings.  ``_NOUN`` is the pool in the words of its errors."""
    _PREFIX = _NOUN = ""

    def __init__(self, tableau: Tableau, handle, count: int):
        self._t, self._p, self.count = tableau, handle, int(count)

    def _call(self, name, *args):
        if self._p is None:
            raise RelpError(f"the {self._NOUN} is closed")
        if not self._t._h:
            raise RelpError(f"the {self._NOUN}'s tableau is closed")
        self._t._ck(getattr(self._t._lib, name)(self._t._h, self._p, *args))

    def _call_ids(self, name, ids, *args):
        i = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        if i.ndim != 1:
            raise ValueError("ids must be one-dimensional")
        self._call(name, i.ctypes.data, i.shape[0], *args)

    def close(self) -> None:
        if self._p is not None and self._t._h:
            getattr(self._t._lib, self._PREFIX + "_destroy")(self._t._h, self._p)
        self._p = None

    def _add(self, ids) -> None:
        self._call_ids(self._PREFIX + "_add", ids)

    def _set_active(self, ids, flag: bool) -> None:
        self._call_ids(self._PREFIX + "_set_active", ids, 1 if flag else 0)

    def _stats(self) -> Tuple[int, int, int, int]:
        out = (C.c_int64 * 4)()
        self._call(self._PREFIX + "_stats", out)
        return tuple(int(x) for x in out)


class ColumnPool(_DevicePool):
    """A column pool of a ``Tableau`` (``Tableau.pool``): candidate columns resident on the device, priced and added in place.
    Freed by ``close()``, or with the tableau."""
    _PREFIX, _NOUN = "relp_pool", "pool"

    def reduced_costs(self) -> np.ndarray:
        """``d_k = c_k + sum_i (-pi)_i a_k[i]`` of every pool column, active or not, with the bits ``add_columns`` would give the
        column's reduced cost at this moment (relp_pool_reduced_costs); read-only."""
        out = np.zeros(self.count)
        self._call("relp_pool_reduced_costs", out.ctypes.data)
        return out

    def price(self, segments: int = 1, tol: float = 1e-7):
        """Multiple pricing (relp_pool_price): the pool indices cut into ``segments`` equal shares, per share the active column with
        the smallest ``d_k < -tol`` (lowest index among equals).  Returns (ids, d) of the winners, ascending share order."""
        ids = np.zeros(max(int(segments), 1), dtype=np.int32)
        d = np.zeros(max(int(segments), 1))
        found = C.c_int32(0)
        self._call("relp_pool_price", int(segments), float(tol), ids.ctypes.data, d.ctypes.data, C.byref(found))
        return ids[:found.value].copy(), d[:found.value].copy()

    def add(self, ids) -> None:
        """The pool columns ``ids`` join the tableau as ``add_columns`` would add them, in that order (relp_pool_add): column k of
        the list is column ``nr_columns() + k`` (read before the call); their activity flags are cleared."""
        self._add(ids)

    def set_active(self, ids, flag: bool) -> None:
        """The activity flag of the pool columns ``ids`` (relp_pool_set_active): an inactive column is priced but never wins."""
        self._set_active(ids, flag)

    def stats(self) -> Tuple[int, int, int, int]:
        """(pool columns, nonzeros held, entries stored on the device with padding, price calls so far); relp_pool_stats."""
        return self._stats()


def column_generation(tableau: Tableau, pool: ColumnPool, segments: int = 1, tol: float = 1e-7, max_rounds: int = 100,
                      max_iters: int = 1 << 40):
    """The column-generation loop on a phase-2 tableau: ``run`` -> ``pool.price(segments, tol)`` -> ``pool.add(winners)`` until
    nothing prices out, the LP is not optimal or ``max_rounds`` rounds have added columns.  Returns (rounds that added columns,
    columns added, last outcome); the outcome is OPTIMAL only if the last pricing found no candidate."""
    rounds, added = 0, 0
    while True:
        outcome = tableau.run(max_iters)[1]
        if outcome != OPTIMAL:
            return rounds, added, outcome
        ids, _ = pool.price(segments, tol)
        if ids.shape[0] == 0:
            return rounds, added, OPTIMAL
        if rounds >= max_rounds:
            return rounds, added, RUNNING
        pool.add(ids)
        rounds += 1
        added += int(ids.shape[0])


class CutPool(_DevicePool):
    """A cut pool of a ``Tableau`` (``Tableau.cut_pool``): candidate cuts resident on the device, separated and added in place.
    Freed by ``close()``, or with the tableau."""
    _PREFIX, _NOUN = "relp_cutpool", "cut pool"

    def slacks(self) -> np.ndarray:
        """``s_k = rhs_k - g_k' x`` of every pool cut, active or not, at the current vertex (relp_cutpool_slacks): one fma chain
        per cut over its entries in ascending column order; ``s_k < 0`` is a violated cut.  Read-only."""
        out = np.zeros(self.count)
        self._call("relp_cutpool_slacks", out.ctypes.data)
        return out

    def separate(self, segments: int = 1, tol: float = 1e-7, by_efficacy: bool = False):
        """Separation (relp_cutpool_separate): the pool indices cut into ``segments`` equal shares, per share the active cut with
        the smallest key among those with ``s_k < -tol``; the key is ``s_k``, or ``s_k / norm_k`` with ``by_efficacy`` (lowest
        index among equals).  Returns (ids, slacks) of the winners, ascending share order."""
        ids = np.zeros(max(int(segments), 1), dtype=np.int32)
        s = np.zeros(max(int(segments), 1))
        found = C.c_int32(0)
        self._call("relp_cutpool_separate", int(segments), float(tol), 1 if by_efficacy else 0, ids.ctypes.data, s.ctypes.data,
                   C.byref(found))
        return ids[:found.value].copy(), s[:found.value].copy()

    def add(self, ids) -> None:
        """The pool cuts ``ids`` join the tableau as ``add_cuts`` would add them, in that order (relp_cutpool_add): cut k of the
        list is row ``nr_rows() + k`` (read before the call); their activity flags are cleared, and stay cleared when a trial
        that added them is rolled back."""
        self._add(ids)

    def set_active(self, ids, flag: bool) -> None:
        """The activity flag of the pool cuts ``ids`` (relp_cutpool_set_active): an inactive cut has a slack but never wins."""
        self._set_active(ids, flag)

    def stats(self) -> Tuple[int, int, int, int]:
        """(pool cuts, nonzeros held, entries stored on the device with padding, separate calls so far); relp_cutpool_stats."""
        return self._stats()


def row_generation(tableau: Tableau, pool: CutPool, tol: float = 1e-7, per_round: int = 1, max_rounds: int = 100,
                   by_efficacy: bool = False, max_iters: int = 1 << 40):
    """The row-generation loop on a phase-2 tableau at a dual feasible basis: ``run_dual`` -> ``pool.separate(per_round, tol,
    by_efficacy)`` -> ``pool.add(winners)`` until no active pool cut is violated, the LP is not optimal or ``max_rounds`` rounds have
    added cuts.  ``per_round`` is the number of shares of a separation (at most the pool's cuts): a round adds at most that many
    cuts.  Returns (rounds that added cuts, cuts added, objective); the objective is None unless the last separation found no
    violated cut on an optimal tableau."""
    rounds, added = 0, 0
    segments = max(1, min(int(per_round), pool.count))
    while True:
        outcome = tableau.run_dual(max_iters)[1]
        if outcome != OPTIMAL:
            return rounds, added, None
        ids, _ = pool.separate(segments, tol, by_efficacy)
        if ids.shape[0] == 0:
            return rounds, added, tableau.objective_function_value()
        if rounds >= max_rounds:
            return rounds, added, None
        pool.add(ids)
        rounds += 1
        added += int(ids.shape[0])


def gomory_rounds(tableau: Tableau, is_integer=None, max_rounds: int = 20, cuts_per_round: int = 3, kind: int = GOMORY_FRACTIONAL,
                  away: float = 1e-6, max_iters: int = 1 << 40):
    """Rounds of Gomory cuts on an optimal phase-2 tableau.  A round reads ``b`` and the basis, takes the first ``cuts_per_round``
    rows whose basic column is flagged integer (``is_integer`` per provider column of the tableau as it stands -- a cut's slack is
    integer when the cut's columns are --, None = all) and whose fraction lies inside [away, 1 - away], and runs ``gomory_cuts`` ->
    ``add_cuts`` (the cuts made) -> ``run_dual``.  Stops when no such row is left, no cut was made, the LP is infeasible or after
    ``max_rounds`` rounds.  Returns (rounds, cuts added, [objective after each round], last outcome)."""
    rounds, added, objectives, outcome = 0, 0, [], OPTIMAL
    while rounds < max_rounds:
        b, basis = tableau.b(), tableau.basis_indices()
        n = tableau.nr_columns()
        flags = np.ones(n, dtype=np.uint8)             # (behind the caller's flags: the slacks of the cuts added since)
        if is_integer is not None:
            given = np.asarray(is_integer)[:n] != 0
            flags[:given.shape[0]] = given
        fraction = b - np.floor(b)
        rows = [i for i in range(b.shape[0])
                if 0 <= basis[i] < n and flags[basis[i]] and away <= fraction[i] <= 1.0 - away][:cuts_per_round]
        if not rows:
            break
        G, rhs, _, status = tableau.gomory_cuts(rows, flags, kind, away)
        made = status == GOMORY_CUT
        if not made.any():
            break
        tableau.add_cuts(G[made], rhs[made])
        outcome = tableau.run_dual(max_iters)[1]
        rounds += 1
        added += int(made.sum())
        if outcome != OPTIMAL:
            break
        objectives.append(tableau.objective_function_value())
    return rounds, added, objectives, outcome


def solve_relaxation(provider: MatrixData, **config_overrides):
    """SolveRelaxation::solve_relaxation (two_phase/mod.rs:30-76).  Returns (outcome, tableau)."""
    t = Tableau(provider, **config_overrides)
    return t.solve_relaxation(), t


# ---- beyond the reference: one answer, checked, out of several attempts -------------------------------------------------------
# The reference has ONE configuration, solves the data as read and does not check what it returns; in f64 its literal rules miss optima
# the safeguards of relp_robust_config reach, and the other way round, and the PILOT family needs scaling while six other files of its
# Netlib directory are LOST by scaling (absolute tolerances on scaled rows).  `solve_verified` is the union as a procedure: legs of
# (data as read | scaled by MatrixData.scaled, configuration, engine) in a fixed order, each with a pivot and a time budget, and an
# outcome stands only when it verifies -- `optimal` by the residuals of relp_check_basis (B^-1 B = I, basis columns are unit columns,
# b >= 0: the wrong optima of the sweeps all sit on a basis with some b_i <= -0.07), `infeasible` / `unbounded` only when every leg
# has run, none reached a verified optimum, and two engines said so on the data AS READ from a state that passes the first two checks
# (on scaled data two engines agreed on a wrong `infeasible` for WOODW; PILOT87 ends `infeasible` on an exploded tableau).
VERIFY_IDENTITY, VERIFY_BASIC, VERIFY_MIN_B = 1e-5, 1e-3, -1e-6
# ("robust-dantzig": the safeguards with PivotRule::SteepestDescent -- the largest coefficient -- in phase 1 as well, where the
# reference takes FirstProfitableWithMemory: TUFF, DEGEN3, CYCLE cycle for 600,000 pivots under the reference's phase-1 rule, under
# Bland's too, and end after 1,708 / 11,775 / 49,326 pivots with this one; PILOT87 reaches Netlib's 301.71072827 with it.)
VERIFIED_LEGS = (("read", "robust", ENGINE_LU), ("scaled", "robust", ENGINE_LU), ("scaled", "robust-dantzig", ENGINE_LU),
                 ("scaled", "robust-dantzig", ENGINE_TABLEAU), ("read", "robust-dantzig", ENGINE_LU), ("scaled", "robust", ENGINE_REVISED),
                 ("read", "robust", ENGINE_REVISED), ("read", "robust", ENGINE_TABLEAU), ("scaled", "robust", ENGINE_TABLEAU),
                 ("read", "default", ENGINE_LU), ("read", "default", ENGINE_REVISED), ("read", "default", ENGINE_TABLEAU),
                 # (the long leg: twelve times the budgets.  DFL001, 5,934 x 12,092: phase 1 takes 920,000 pivots and the optimum
                 # 1,990,000 -- 230 s on the tableau engine -- where every other leg is cut off)
                 ("read", "robust-dantzig", ENGINE_TABLEAU, 12))
_ENGINE_NAMES = {ENGINE_REVISED: "revised", ENGINE_TABLEAU: "tableau", ENGINE_LU: "lu"}


def solve_verified(provider: MatrixData, pivots_per_leg: Optional[int] = None, seconds_per_leg: float = 60.0, legs=VERIFIED_LEGS):
    """Returns (outcome, tableau or None, report).  `report["verified"]` says whether the outcome passed its check; `report["legs"]`
    lists what every leg did.  The tableau of the leg that was accepted is returned open (close it); the others are closed.  When
    the accepted leg ran on scaled data (`report["scaled"]`) the objective value is still the provider's; a solution is brought
    back by `provider.unscale_bfs(t.current_bfs(), report["row_scale"], report["column_scale"])`."""
    import time
    budget = pivots_per_leg if pivots_per_leg is not None else 30 * (int(provider.nr_rows) + int(provider.nr_columns))
    report = {"legs": [], "verified": False, "scaled": False}
    scaled = None
    said = {}                                           # infeasible / unbounded -> engines that said so on the data as read
    last = RUNNING
    for entry in legs:
        data, cfg_name, kind = entry[:3]
        times = entry[3] if len(entry) > 3 else 1                # (a long leg: `times` the pivot and time budgets)
        leg = {"data": data, "config": cfg_name, "engine": _ENGINE_NAMES[kind]}
        report["legs"].append(leg)
        t0 = time.perf_counter()
        if data == "scaled" and scaled is None:
            scaled = provider.scaled()
        if cfg_name == "robust":
            cfg = robust_config(engine=kind)
        elif cfg_name == "robust-dantzig":
            cfg = robust_config(engine=kind, phase_one_rule=STEEPEST_DESCENT, phase_two_rule=STEEPEST_DESCENT)
        else:
            cfg = default_config(engine=kind)
        try:
            t = Tableau(scaled[0] if data == "scaled" else provider, config=cfg)
        except RelpError as e:
            leg["outcome"] = "create_failed: " + str(e)[:120]
            continue
        try:
            oc, total = RUNNING, 0
            while total < times * budget and time.perf_counter() - t0 < times * seconds_per_leg:
                done, oc = t.run(min(20000, times * budget - total))
                total += done
                if oc not in (RUNNING, PHASE_ONE_DONE):
                    break
            leg["pivots"] = total
            leg["outcome"] = OUTCOME_NAMES.get(oc, str(oc)) if oc not in (RUNNING, PHASE_ONE_DONE) else "limit"
            last = oc
            if oc == OPTIMAL:
                ident, basic, min_b = t.check_basis()
                leg["check_basis"] = [ident, basic, min_b]
                if ident <= VERIFY_IDENTITY and basic <= VERIFY_BASIC and min_b >= VERIFY_MIN_B:
                    report["verified"] = True
                    report["scaled"] = data == "scaled"
                    if data == "scaled":
                        report["row_scale"], report["column_scale"] = scaled[1], scaled[2]
                    return OPTIMAL, t, report
            elif oc in (INFEASIBLE, UNBOUNDED) and data == "read":
                # (a claim counts only from a state that is still a basis: PILOT87 on the tableau engine ends `infeasible` with
                # a phase-1 objective of 1e302 and then inf)
                ident, basic, min_b = t.check_basis()
                leg["check_basis"] = [ident, basic, min_b]
                if ident <= VERIFY_IDENTITY and basic <= VERIFY_BASIC and np.isfinite(t.objective_function_value()):
                    said.setdefault(oc, set()).add(kind)
        except RelpError as e:
            leg["outcome"] = "error: " + str(e)[:120]
        t.close()
    for oc, engines in said.items():
        if len(engines) >= 2:
            report["verified"] = True
            return oc, None, report
    return last, None, report
