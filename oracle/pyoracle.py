"""oracle/pyoracle.py -- Python face of the CPU oracle (ctypes over oracle/liboracle.so + NumPy).

TEST INFRASTRUCTURE ONLY: imported by tests/, by __graft_entry__.smoke() and by bench.py's
`cpu_baseline` leg.  The product package (rocco_amd/) never imports this module.

Function names and return conventions mirror the reference so parity tests read like the
reference's own tests:
    rocco/dp.py:16-34    objective_value
    rocco/dp.py:37-46    build_switch_costs
    rocco/dp.py:49-86    solve_penalized_chain
    rocco/dp.py:89-164   calibrate_selection_penalty
    rocco/dp.py:167-228  solve_chrom_exact
    rocco/rocco.py:74-95, 139-191, 194-240   BED record merge / per-chromosome BED / combine
    rocco/rocco.py:243-304                   score_central_tendency_chrom (median branch)
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liboracle.so")

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_u8_p = ctypes.POINTER(ctypes.c_uint8)


class DeltaStats(ctypes.Structure):
    _fields_ = [
        ("count", ctypes.c_longlong),
        ("uncertain", ctypes.c_longlong),
        ("effect", ctypes.c_longlong),
        ("max_run", ctypes.c_longlong),
        ("overflow", ctypes.c_int),
    ]


class WindowStats(ctypes.Structure):
    _fields_ = [
        ("count_lo", ctypes.c_longlong),
        ("count_hi", ctypes.c_longlong),
        ("n_diff", ctypes.c_longlong),
        ("diff_adjacent", ctypes.c_int),
        ("overflow", ctypes.c_int),
        ("max_run", ctypes.c_longlong),
    ]


class WindowDiff(ctypes.Structure):
    _fields_ = [
        ("locus", ctypes.c_longlong),
        ("margin_lo", ctypes.c_double),
        ("margin_hi", ctypes.c_double),
        ("run", ctypes.c_longlong),
        ("cls_lo", ctypes.c_int),
        ("cls_hi", ctypes.c_int),
    ]


class Noise(ctypes.Structure):
    _fields_ = [
        ("p16", ctypes.c_longlong),
        ("npos", ctypes.c_longlong),
        ("tau0", ctypes.c_double),
        ("tau_step", ctypes.c_double),
        ("guard", ctypes.c_double),
    ]


def build(force: bool = False) -> str:
    """Compile oracle/liboracle.so (and oracle/_ref when the reference is mounted)."""
    # (make compares the library with its sources: a library left by an older tree is rebuilt, a current one is kept)
    subprocess.run(["make", "-C", _HERE, "liboracle.so"] + (["-B"] if force else []), check=True, capture_output=True)
    if os.path.isdir("/root/reference"):
        subprocess.run(["make", "-C", _HERE, "ref"], check=False, capture_output=True)
    return _LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.oracle_solve_penalized_chain_f64.restype = ctypes.c_int
        _lib.oracle_solve_penalized_chain_f64.argtypes = [
            _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_double,
            _c_u8_p, _c_double_p, ctypes.POINTER(ctypes.c_longlong)]
        _lib.oracle_calibrate_selection_penalty_f64.restype = ctypes.c_int
        _lib.oracle_calibrate_selection_penalty_f64.argtypes = [
            _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_longlong,
            ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, _c_double_p,
            _c_u8_p, _c_double_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)]
        _lib.oracle_objective_value_f64.restype = ctypes.c_double
        _lib.oracle_objective_value_f64.argtypes = [
            _c_u8_p, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t]
        _lib.oracle_global_exponent.restype = ctypes.c_int
        _lib.oracle_global_exponent.argtypes = [
            _c_double_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
            ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
        _lib.oracle_binade_map.restype = ctypes.c_int
        _lib.oracle_binade_map.argtypes = [
            _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_double, ctypes.c_int,
            ctypes.c_double, _c_u8_p]
        _lib.oracle_delta_chain_f64.restype = ctypes.c_int
        _lib.oracle_delta_chain_f64.argtypes = [
            _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_double, ctypes.c_int,
            ctypes.c_double, ctypes.c_double, _c_u8_p, _c_u8_p, ctypes.POINTER(DeltaStats)]
        _lib.oracle_delta_window_f64.restype = ctypes.c_int
        _lib.oracle_delta_window_f64.argtypes = [
            _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_double,
            ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_u8_p, _c_u8_p,
            ctypes.POINTER(WindowStats), ctypes.POINTER(WindowDiff), ctypes.c_int]
        _lib.oracle_median_columns.restype = ctypes.c_int
        _lib.oracle_median_columns.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, _c_double_p]
        _lib.oracle_score_centered_wls_f64.restype = ctypes.c_int
        _lib.oracle_score_centered_wls_f64.argtypes = [
            _c_double_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_double,
            ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
            _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]
        _lib.oracle_score_centered_wls_given_variances_f64.restype = ctypes.c_int
        _lib.oracle_score_centered_wls_given_variances_f64.argtypes = [
            _c_double_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_double,
            ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
            _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]
        _lib.oracle_wls_spatial_window.restype = ctypes.c_size_t
        _lib.oracle_wls_spatial_window.argtypes = [ctypes.c_size_t, ctypes.c_int]
        _lib.oracle_rolling_ar1_innovation_variance_starts_f64.restype = ctypes.c_int
        _lib.oracle_rolling_ar1_innovation_variance_starts_f64.argtypes = [
            _c_double_p, ctypes.c_size_t, ctypes.c_size_t, _c_double_p]
        _lib.oracle_monotone_variance_trend_f64.restype = ctypes.c_int
        _lib.oracle_monotone_variance_trend_f64.argtypes = [_c_double_p, _c_double_p, ctypes.c_size_t, _c_double_p]
        _lib.oracle_crossfit_whittaker_baseline_matrix_f64.restype = ctypes.c_int
        _lib.oracle_crossfit_whittaker_baseline_matrix_f64.argtypes = [
            _c_double_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, _c_double_p]
    return _lib


def _dptr(a: Optional[np.ndarray]):
    if a is None:
        return ctypes.cast(None, _c_double_p)
    return a.ctypes.data_as(_c_double_p)


def _u8ptr(a: Optional[np.ndarray]):
    if a is None:
        return ctypes.cast(None, _c_u8_p)
    return a.ctypes.data_as(_c_u8_p)


def _check(rc: int) -> None:
    if rc == -1:
        raise MemoryError("oracle allocation failed")
    if rc != 0:
        raise ValueError(f"oracle rejected the arguments (status {rc})")


# --------------------------------------------------------------------------------------------
# dp.py surface
# --------------------------------------------------------------------------------------------

def objective_value(solution, scores, switch_costs) -> float:
    """rocco/dp.py:16-34, restated with the same NumPy expressions (BLAS dot order)."""
    solution_ = np.asarray(solution, dtype=np.float64)
    scores_ = np.asarray(scores, dtype=np.float64)
    if np.isscalar(switch_costs):
        costs_ = np.full(max(solution_.shape[0] - 1, 0), float(switch_costs), dtype=np.float64)
    else:
        costs_ = np.asarray(switch_costs, dtype=np.float64)
    penalty = 0.0
    if solution_.shape[0] > 1:
        penalty = float(costs_ @ np.abs(np.diff(solution_, 1)))
    return float(-(scores_ @ solution_) + penalty)


def build_switch_costs(scores, gamma: float = 1.0) -> np.ndarray:
    """rocco/dp.py:37-46."""
    scores_ = np.asarray(scores, dtype=np.float64)
    if scores_.ndim != 1:
        raise ValueError("`scores` must be a one-dimensional array")
    if scores_.shape[0] <= 1:
        return np.zeros(0, dtype=np.float64)
    return np.full(scores_.shape[0] - 1, float(gamma), dtype=np.float64)


def _prep(scores, switch_costs) -> Tuple[np.ndarray, np.ndarray]:
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    costs_ = np.ascontiguousarray(switch_costs, dtype=np.float64)
    if scores_.ndim != 1:
        raise ValueError("`scores` must be one-dimensional")
    if costs_.ndim != 1:
        raise ValueError("`switch_costs` must be one-dimensional")
    n = scores_.shape[0]
    if n <= 0:
        raise ValueError("`scores` cannot be empty")
    if n > 1 and costs_.shape[0] != n - 1:
        raise ValueError("`switch_costs` must have length len(scores) - 1")
    return scores_, costs_


def solve_penalized_chain(scores, switch_costs, selection_penalty: float):
    """rocco/dp.py:49-86 -> rocco/_chain_dp.c:9-213.  Returns (uint8[n], value, count)."""
    scores_, costs_ = _prep(scores, switch_costs)
    n = scores_.shape[0]
    solution = np.zeros(n, dtype=np.uint8)
    value = ctypes.c_double(0.0)
    count = ctypes.c_longlong(0)
    _check(lib().oracle_solve_penalized_chain_f64(
        _dptr(scores_), _dptr(costs_) if n > 1 else _dptr(None), 0.0, n, float(selection_penalty),
        _u8ptr(solution), ctypes.byref(value), ctypes.byref(count)))
    return solution, float(value.value), int(count.value)


def calibrate_selection_penalty(scores, switch_costs, target_count: int, max_iter: int = 60,
                                return_evaluations: bool = False):
    """rocco/dp.py:89-164.  Returns (upper, best_solution, best_value, best_count)."""
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    costs_ = np.ascontiguousarray(switch_costs, dtype=np.float64)
    n = scores_.shape[0]
    if n == 0:
        raise ValueError("`scores` cannot be empty")
    solution = np.zeros(n, dtype=np.uint8)
    penalty = ctypes.c_double(0.0)
    value = ctypes.c_double(0.0)
    count = ctypes.c_longlong(0)
    evals = ctypes.c_int(0)
    # np.min / np.max / np.sum exactly as dp.py:110-111 calls them
    _check(lib().oracle_calibrate_selection_penalty_f64(
        _dptr(scores_), _dptr(costs_) if n > 1 else _dptr(None), 0.0, n, int(target_count),
        int(max_iter), float(np.sum(costs_)), float(np.min(scores_)), float(np.max(scores_)),
        ctypes.byref(penalty), _u8ptr(solution), ctypes.byref(value), ctypes.byref(count),
        ctypes.byref(evals)))
    out = (float(penalty.value), solution, float(value.value), int(count.value))
    if return_evaluations:
        return out + (int(evals.value),)
    return out


def solve_chrom_exact(scores, budget: Optional[float] = None, gamma: float = 1.0,
                      selection_penalty: Optional[float] = None, return_details: bool = False):
    """rocco/dp.py:167-228."""
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    switch_costs = build_switch_costs(scores_, gamma=gamma)
    if selection_penalty is None:
        if budget is None:
            penalty_ = 0.0
            solution, penalized, count = solve_penalized_chain(scores_, switch_costs, penalty_)
        else:
            target_count = int(np.floor(len(scores_) * float(budget)))
            penalty_, solution, penalized, count = calibrate_selection_penalty(
                scores_, switch_costs, target_count=target_count)
    else:
        penalty_ = float(selection_penalty)
        solution, penalized, count = solve_penalized_chain(scores_, switch_costs, penalty_)
    objective = objective_value(solution, scores_, switch_costs)
    if not return_details:
        return solution.astype(np.uint8, copy=False), objective
    return solution.astype(np.uint8, copy=False), objective, {
        "penalized_objective": float(penalized),
        "selected_count": int(count),
        "selected_fraction": float(count / len(scores_)),
        "selection_penalty": float(penalty_),
    }


# --------------------------------------------------------------------------------------------
# delta-form recursion (sequential definition of the GPU fast path)
# --------------------------------------------------------------------------------------------

def grid_exponent(cmax: float, smin: float, smax: float) -> int:
    """qexp such that every value of magnitude <= 8 R is exact on the grid 2^qexp, with
    R = cmax + (smax - smin) + 2 (penalties are evaluated within [smin - 1, smax + 1])."""
    r = float(cmax) + (float(smax) - float(smin)) + 2.0
    import math
    return int(math.ceil(math.log2(8.0 * r))) - 52


def _costs(gamma_or_costs):
    if np.isscalar(gamma_or_costs):
        return None, float(gamma_or_costs), float(gamma_or_costs)
    c = np.ascontiguousarray(gamma_or_costs, dtype=np.float64)
    return c, 0.0, float(c.max()) if c.size else 0.0


def binade_map(scores, gamma_or_costs, lambda_ref: float, margin: float, qexp: int = None) -> np.ndarray:
    """Per-chunk binade codes at penalty lambda_ref (oracle_binade_map)."""
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    n = scores_.shape[0]
    costs_, gamma, cmax = _costs(gamma_or_costs)
    if qexp is None:
        qexp = grid_exponent(cmax, scores_.min(), scores_.max())
    emap = np.zeros((n + 31) // 32, dtype=np.uint8)
    _check(lib().oracle_binade_map(_dptr(scores_), _dptr(costs_), gamma, n, float(lambda_ref), int(qexp),
                                   float(margin), _u8ptr(emap)))
    return emap


def delta_chain(scores, gamma_or_costs, selection_penalty: float, qexp: int = None, emap=None,
                want_solution: bool = True):
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    n = scores_.shape[0]
    costs_, gamma, cmax = _costs(gamma_or_costs)
    if qexp is None:
        qexp = grid_exponent(cmax, scores_.min(), scores_.max())
    solution = np.zeros(n, dtype=np.uint8) if want_solution else None
    emap_ = None if emap is None else np.ascontiguousarray(emap, dtype=np.uint8)
    stats = DeltaStats()
    _check(lib().oracle_delta_chain_f64(_dptr(scores_), _dptr(costs_), gamma, n, float(selection_penalty),
                                        int(qexp), cmax, float(np.max(np.abs(scores_))), _u8ptr(emap_),
                                        _u8ptr(solution), ctypes.byref(stats)))
    return solution, {"count": stats.count, "uncertain": stats.uncertain, "effect": stats.effect,
                      "max_run": stats.max_run, "overflow": bool(stats.overflow)}


def delta_window(scores, gamma_or_costs, lambda_lo: float, lambda_hi: float, qexp: int = None, emap=None,
                 diff_capacity: int = 16):
    scores_ = np.ascontiguousarray(scores, dtype=np.float64)
    n = scores_.shape[0]
    costs_, gamma, cmax = _costs(gamma_or_costs)
    if qexp is None:
        qexp = grid_exponent(cmax, scores_.min(), scores_.max())
    solution = np.zeros(n, dtype=np.uint8)
    emap_ = None if emap is None else np.ascontiguousarray(emap, dtype=np.uint8)
    stats = WindowStats()
    diffs = (WindowDiff * max(1, diff_capacity))()
    _check(lib().oracle_delta_window_f64(_dptr(scores_), _dptr(costs_), gamma, n, float(lambda_lo),
                                         float(lambda_hi), int(qexp), cmax,
                                         float(np.max(np.abs(scores_))), _u8ptr(emap_), _u8ptr(solution),
                                         ctypes.byref(stats), diffs, int(diff_capacity)))
    listed = min(int(stats.n_diff), diff_capacity)
    return solution, {"count_lo": stats.count_lo, "count_hi": stats.count_hi, "n_diff": stats.n_diff,
                      "diff_adjacent": bool(stats.diff_adjacent), "overflow": bool(stats.overflow),
                      "max_run": stats.max_run,
                      "diffs": [{"locus": int(d.locus), "margin_lo": d.margin_lo, "margin_hi": d.margin_hi,
                                 "run": int(d.run), "cls_lo": d.cls_lo, "cls_hi": d.cls_hi}
                                for d in diffs[:listed]]}


# --------------------------------------------------------------------------------------------
# scoring and BED (rocco/rocco.py)
# --------------------------------------------------------------------------------------------

def score_central_tendency_chrom(chrom_matrix, method="quantile", quantile=0.50, tprop=0.05, power=1.0):
    """rocco/rocco.py:243-304, median branch only (the branch rocco.py:983-991 reaches)."""
    m = np.asarray(chrom_matrix)
    if m.ndim != 2:
        raise ValueError("`chrom_matrix` must be a 2D array.")
    method_ = str(method).strip().lower().replace("-", "").replace("_", "")
    if method_ != "quantile" or quantile != 0.50 or power != 1.0:
        raise NotImplementedError("oracle restates the median branch only")
    if m.shape[0] == 1:
        return np.asarray(m[0, :], dtype=float)
    is_f32 = m.dtype == np.float32
    m_ = np.ascontiguousarray(m, dtype=np.float32 if is_f32 else np.float64)
    out = np.empty(m_.shape[1], dtype=np.float64)
    _check(lib().oracle_median_columns(m_.ctypes.data_as(ctypes.c_void_p), int(is_f32), m_.shape[0],
                                       m_.shape[1], _dptr(out)))
    return out


Record = Tuple[str, int, int]


def merge_bed_records(records: Sequence[Record], min_length_bp: Optional[int] = None) -> List[Record]:
    """rocco/rocco.py:74-95: sort by (chrom string, start, end), merge when start <= previous end,
    then drop records shorter than min_length_bp."""
    out: List[List] = []
    for chrom, start, end in sorted(records, key=lambda r: (r[0], r[1], r[2])):
        if out and chrom == out[-1][0] and int(start) <= int(out[-1][2]):
            out[-1][2] = max(int(out[-1][2]), int(end))
        else:
            out.append([chrom, int(start), int(end)])
    return [(str(c), int(s), int(e)) for c, s, e in out
            if min_length_bp is None or (int(e) - int(s)) >= int(min_length_bp)]


def chrom_solution_records(chromosome, intervals, solution, check_gaps_intervals=True,
                           min_length_bp=None) -> List[Record]:
    """rocco/rocco.py:139-191 up to (not including) the file write: loci 0..n-2 with
    solution > 0.5 become (intervals[i], intervals[i+1]); the last locus is never emitted."""
    if len(intervals) != len(solution):
        raise ValueError("Intervals and solution must have the same length")
    if check_gaps_intervals and len(set(np.diff(intervals))) > 1:
        raise ValueError("Intervals must be contiguous")
    recs = [(str(chromosome), int(intervals[i]), int(intervals[i + 1]))
            for i in range(len(intervals) - 1) if solution[i] > 0.50]
    return merge_bed_records(recs, min_length_bp=min_length_bp)


def bed_text(records: Sequence[Record], name_features: bool = False) -> str:
    """rocco/rocco.py:98-110."""
    if name_features:
        return "".join(f"{c}\t{s}\t{e}\t{c}_{s}_{e}\n" for c, s, e in records)
    return "".join(f"{c}\t{s}\t{e}\n" for c, s, e in records)


def combine_records(per_chrom_records: Sequence[Sequence[Record]]) -> List[Record]:
    """rocco/rocco.py:194-240 on in-memory records."""
    allr: List[Record] = []
    for recs in per_chrom_records:
        allr.extend(recs)
    return merge_bed_records(allr)


def crossfit_whittaker_baseline(values, penalty_lambda: float) -> np.ndarray:
    """rocco/_baseline.c:16-104 over rocco/native/baseline_backend.c:252-334 (1-D or 2-D input)."""
    m = np.ascontiguousarray(values, dtype=np.float64)
    if m.ndim not in (1, 2):
        raise ValueError("`values` must be one-dimensional or two-dimensional")
    out = np.empty_like(m)
    rows, cols = (1, m.shape[0]) if m.ndim == 1 else m.shape
    if m.size:
        _check(lib().oracle_crossfit_whittaker_baseline_matrix_f64(
            _dptr(m), rows, cols, float(penalty_lambda), _dptr(out)))
    return out


def wls_spatial_window(n: int, requested: int = 31) -> int:
    """rocco/native/wls_backend.c:232-260: odd, at least 5, at most n; 0 for fewer than 5 loci."""
    return int(lib().oracle_wls_spatial_window(int(n), int(requested)))


def rolling_variances_at_starts(centered_matrix, spatial_window: int = 31):
    """rocco/native/wls_backend.c:610-726 on every row: the AR(1) innovation variance of every window BY ITS START
    POSITION, [K, n - window + 1] (locus i of the scoring reads start clamp(i - window // 2, 0, n - window)); None where
    the row has no window (fewer than 5 loci)."""
    m = np.ascontiguousarray(centered_matrix, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] == 0 or m.shape[1] == 0:
        raise ValueError("`centered_matrix` must be a non-empty two-dimensional array")
    K, n = m.shape
    window = wls_spatial_window(n, spatial_window)
    if window == 0:
        return None
    out = np.empty((K, n - window + 1), dtype=np.float64)
    for k in range(K):
        _check(lib().oracle_rolling_ar1_innovation_variance_starts_f64(_dptr(m[k]), n, window, _dptr(out[k])))
    return out


def monotone_variance_trend(covariate, raw_variance) -> np.ndarray:
    """rocco/native/wls_backend.c:394-608 on one row: the monotone trend of the variances over |covariate|."""
    cov = np.ascontiguousarray(covariate, dtype=np.float64)
    raw = np.ascontiguousarray(raw_variance, dtype=np.float64)
    if cov.ndim != 1 or raw.shape != cov.shape:
        raise ValueError("`covariate` and `raw_variance` must be one-dimensional and of one length")
    out = np.empty(cov.shape[0], dtype=np.float64)
    _check(lib().oracle_monotone_variance_trend_f64(_dptr(cov), _dptr(raw), cov.shape[0], _dptr(out)))
    return out


def score_centered_wls(centered_matrix, lower_bound_z: float = 1.0, prior_df: float = 5.0, min_effect=None,
                       spatial_window: int = 31, precision_floor_ratio: float = 0.01, variances=None):
    """rocco/_wls.c `score_centered_wls` over rocco/native/wls_backend.c:744-947: returns
    (scores, mean, raw_variance, prior_variance, moderated_variance, standard_error, total_df, window).
    `variances` [K, n - window + 1]: every row's rolling variances by window start, dictated by the caller in place of
    `rolling_variances_at_starts` (the reference has no such entry; everything behind the variances is its code path)."""
    m = np.ascontiguousarray(centered_matrix, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] == 0 or m.shape[1] == 0:
        raise ValueError("`centered_matrix` must be a non-empty two-dimensional array")
    K, n = m.shape
    given = None
    if variances is not None:
        window = wls_spatial_window(n, spatial_window)
        given = np.ascontiguousarray(variances, dtype=np.float64)
        if window == 0 or given.shape != (K, n - window + 1):
            raise ValueError("`variances` must be [K, n - window + 1]")
    tracks = [np.empty(n, dtype=np.float64) for _ in range(6)]
    df, win = ctypes.c_double(), ctypes.c_int()
    _check(lib().oracle_score_centered_wls_given_variances_f64(
        _dptr(m), K, n, float(lower_bound_z), float(prior_df), float(0.0 if min_effect is None else min_effect),
        0 if min_effect is None else 1, int(spatial_window), float(precision_floor_ratio), _dptr(given),
        *[_dptr(t) for t in tracks], ctypes.byref(df), ctypes.byref(win)))
    mean, raw, prior, mod, se, scores = tracks
    return scores, mean, raw, prior, mod, se, float(df.value), int(win.value)


def score_loci_wls(chrom_matrix, lower_bound_z: float = 1.0, prior_df: float = 5.0, min_effect=None,
                   precision_floor_ratio: float = 0.01, log_matrix=None):
    """rocco/inference.py:302-379 restated over the oracle's backends: NumPy for the log scale (40-47), the
    pilot offset (330-331) and the subtraction (335); `crossfit_whittaker_baseline` (185-229) and
    `score_centered_wls` (231-299) for the rest.  `log_matrix` replaces the log-scaled matrix (tests use it
    to separate the one-ulp freedom of log2 from everything downstream).  Returns (scores, details)."""
    if log_matrix is None:
        counts = np.asarray(chrom_matrix, dtype=np.float64)
        if np.any(~np.isfinite(counts)):
            raise ValueError("`chrom_matrix` contains non-finite values")
        matrix = np.log2(np.clip(counts, 0.0, None) + 1.0)
    else:
        matrix = np.asarray(log_matrix, dtype=np.float64)
    if matrix.ndim != 2 or matrix.shape[0] == 0 or matrix.shape[1] == 0:
        raise ValueError("`chrom_matrix` must be a non-empty two-dimensional array")
    global_centered = matrix - np.median(matrix, axis=1, keepdims=True)
    n = matrix.shape[1]
    window, lam = 0, 0.0
    if n >= 25:  # inference.py:49-62 with target_window 101
        window = min(101, n)
        if window % 2 == 0:
            window = window - 1 if window == n else window + 1
        block = max(3, window)
        block += 1 if block % 2 == 0 else 0
        lam = float(7.0 * ((float(block) * 0.15915494) ** 4))  # inference.py:65-76
        centered = global_centered - crossfit_whittaker_baseline(global_centered, lam)
    else:
        centered = global_centered - np.zeros_like(global_centered)
    scores, mean, raw, prior, mod, se, df, win = score_centered_wls(
        centered, lower_bound_z=lower_bound_z, prior_df=prior_df, min_effect=min_effect, spatial_window=31,
        precision_floor_ratio=max(precision_floor_ratio, 0.0))
    details = {"input_scale": "log2p1", "local_baseline_window": int(window), "local_baseline_lambda": lam,
               "mean": mean, "raw_variance": raw, "prior_variance": prior, "moderated_variance": mod,
               "standard_error": se, "z_scores": mean / np.maximum(se, 1.0e-8),
               "min_effect": float(0.0 if min_effect is None else max(min_effect, 0.0)),
               "precision_floor_ratio": float(max(precision_floor_ratio, 0.0)), "prior_spatial_window": int(win),
               "degrees_of_freedom": np.full(n, float(df)), "centered_matrix": centered}
    return scores, details


def narrowpeak_summit_track(intervals, effect_mean):
    """rocco/rocco.py:809-835 without the temporary file: (starts, centers, float32 mean) or None."""
    intervals_ = np.asarray(intervals, dtype=np.int64)
    effect_mean_ = np.asarray(effect_mean, dtype=np.float32)
    usable = int(min(max(intervals_.shape[0] - 1, 0), effect_mean_.shape[0]))
    if usable <= 0:
        return None
    centers = (intervals_[:usable].astype(np.int64) + intervals_[1:usable + 1].astype(np.int64)) // 2
    return intervals_[:usable].copy(), centers, effect_mean_[:usable].copy()


def narrowpeak_summit_offsets(records: Sequence[Record], tracks: Dict[str, Optional[tuple]]) -> List[Tuple[str, int]]:
    """rocco/rocco.py:838-872 as a list of (peak name, offset); `tracks[chrom]` is the summit track or None."""
    out = []
    for chrom, start, end in records:
        summit_offset = -1
        track = tracks.get(chrom)
        peak_length = int(end) - int(start)
        if track is not None and peak_length > 0:
            starts, centers = np.asarray(track[0], dtype=np.int64), np.asarray(track[1], dtype=np.int64)
            mean_track = np.asarray(track[2], dtype=np.float64)
            left = int(np.searchsorted(starts, int(start), side="left"))
            right = int(np.searchsorted(starts, int(end), side="left"))
            if right > left:
                local_mean = mean_track[left:right]
                if np.any(np.isfinite(local_mean)):
                    local_idx = int(np.nanargmax(local_mean))
                    summit_bp = int(centers[left + local_idx])
                    summit_offset = int(np.clip(summit_bp - int(start), 0, max(peak_length - 1, 0)))
        out.append((f"{chrom}_{start}_{end}", summit_offset))
    return out


def assemble_chrom_matrix(interval_matrix, vals_matrix, track_type: str = "bam", low_memory: bool = False,
                          chromosome: str = ""):
    """The tail of generate_chrom_matrix (rocco/readtracks.py:614-633), NumPy statement by NumPy statement."""
    common_intervals = np.sort(np.unique(np.concatenate(interval_matrix, axis=0)))
    if track_type == "bigwig" and common_intervals.size > 1:
        if np.unique(np.diff(common_intervals)).size != 1:
            raise ValueError(f"bigWig inputs for {chromosome} do not share one fixed binning scheme")
    matrix_dtype = np.float32 if low_memory else np.float64
    count_matrix = np.zeros((len(interval_matrix), len(common_intervals)), dtype=matrix_dtype)
    for i, (intervals_, vals_) in enumerate(zip(interval_matrix, vals_matrix)):
        idx = np.searchsorted(common_intervals, intervals_)
        count_matrix[i, idx] = np.asarray(vals_, dtype=matrix_dtype)
    return np.array(common_intervals).astype(int), count_matrix


def fit_budget_null_residual_template(centered_matrix, lower_bound_z=1.0, prior_df=5.0, min_effect=None,
                                      precision_floor_ratio=0.01):
    """rocco/inference.py:688-722: (residual_template, observed_scores, positive_consensus)."""
    centered = np.asarray(centered_matrix, dtype=np.float64)
    res = score_centered_wls(centered, lower_bound_z=lower_bound_z, prior_df=prior_df, min_effect=min_effect,
                             spatial_window=31, precision_floor_ratio=max(precision_floor_ratio, 0.0))
    positive_consensus = np.clip(res[1], 0.0, None)
    return centered - positive_consensus[None, :], res[0].astype(np.float64), positive_consensus


def compute_budget_null_draw(residual_template, wild_weights, lower_bound_z, prior_df, min_effect,
                             precision_floor_ratio, null_center, null_soft_scale, null_threshold):
    """rocco/inference.py:656-685 given the draw's multipliers (one row per sample)."""
    bootstrap_centered = np.asarray(residual_template, dtype=np.float64) * np.asarray(wild_weights, dtype=np.float64)
    scores = score_centered_wls(bootstrap_centered, lower_bound_z=lower_bound_z, prior_df=prior_df,
                                min_effect=(None if min_effect is None else float(max(min_effect, 0.0))),
                                spatial_window=31, precision_floor_ratio=max(precision_floor_ratio, 0.0))[0]
    residual = np.asarray(scores, dtype=np.float64) - null_center
    positive = np.clip(residual, 0.0, None)
    return (float(np.mean(positive)), float(np.mean(positive / null_soft_scale)), float(np.mean(positive > 0.0)),
            float(np.mean(scores > null_threshold)))


def bigwig_dense_fill(starts, ends, vals, const_scale: float = 1.0, round_digits: int = 5, bigwig_file: str = "",
                      chromosome: str = ""):
    """get_bigwig_chrom_scores after the file has been read (rocco/readtracks.py:141-186), NumPy statement by
    NumPy statement."""
    starts = np.asarray(starts, dtype=np.int64)
    ends = np.asarray(ends, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    if not np.all(np.isfinite(vals)):
        raise ValueError(f"bigWig values for {bigwig_file} {chromosome} contain non-finite entries")
    widths = ends - starts
    if np.any(widths <= 0):
        raise ValueError(f"bigWig intervals for {bigwig_file} {chromosome} contain non-positive widths")
    step = int(widths[0])
    if np.any(widths != step):
        raise ValueError(f"bigWig file {bigwig_file} uses variable-width bins on {chromosome}; ROCCO expects a "
                         "fixed-width binning scheme")
    offset = int(starts[0])
    idx = starts - offset
    if np.any(idx % step != 0):
        raise ValueError(f"bigWig starts for {bigwig_file} {chromosome} are not aligned to a single fixed binning scheme")
    idx = (idx // step).astype(np.int64, copy=False)
    if np.unique(idx).size != idx.size:
        raise ValueError(f"bigWig file {bigwig_file} has overlapping or duplicate bins on {chromosome}")
    full_intervals = np.arange(int(starts[0]), int(starts[-1]) + step, step, dtype=np.int64)
    full_vals = np.zeros(full_intervals.size, dtype=np.float64)
    full_vals[idx] = vals
    if const_scale >= 0:
        full_vals = full_vals * float(const_scale)
    return full_intervals.astype(int), np.round(full_vals, round_digits)


# --------------------------------------------------------------------------------------------
# budget / switch-cost estimation and the composed driver (oracle/budget_oracle.py), under this module's name
# --------------------------------------------------------------------------------------------
from budget_oracle import (  # noqa: E402,F401
    build_chrom_cache,
    effective_sample_size,
    estimate_budget_nonnull_fraction_from_score_track,
    estimate_budget_nonnull_fraction_from_wild_bootstrap_null,
    estimate_empirical_bayes_budgets,
    resolve_budgets,
    resolve_chrom_gamma,
    run_chromosomes,
)
