"""ctypes wrapper for tests/host_logic/libhostlogic.so (product search logic on the CPU oracle)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_logic")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", _HERE], check=True, capture_output=True)
        _lib = ctypes.CDLL(os.path.join(_HERE, "libhostlogic.so"))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.hostlogic_calibrate.restype = ctypes.c_int
        _lib.hostlogic_calibrate.argtypes = [
            dp, dp, ctypes.c_double, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_double, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), dp, dp,
            ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
        _lib.hostlogic_solve_fixed.restype = ctypes.c_int
        _lib.hostlogic_solve_fixed.argtypes = [
            dp, dp, ctypes.c_double, ctypes.c_size_t, ctypes.c_double,
            ctypes.POINTER(ctypes.c_uint8), dp, ctypes.POINTER(ctypes.c_longlong),
            ctypes.POINTER(ctypes.c_longlong)]
        llp = ctypes.POINTER(ctypes.c_longlong)
        _lib.hostlogic_model_chain_layout.restype = None
        _lib.hostlogic_model_chain_layout.argtypes = [
            ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int), llp, llp, llp, llp, llp]
    return _lib


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


def calibrate(scores, gamma_or_costs, target, max_iter=60, spec_depth=2, force_exact=False):
    s = np.ascontiguousarray(scores, dtype=np.float64)
    n = s.shape[0]
    if np.isscalar(gamma_or_costs):
        costs, gamma = None, float(gamma_or_costs)
        total = float(np.sum(np.full(max(n - 1, 0), gamma)))
    else:
        costs, gamma = np.ascontiguousarray(gamma_or_costs, dtype=np.float64), 0.0
        total = float(np.sum(costs))
    sol = np.zeros(n, dtype=np.uint8)
    pen, val = ctypes.c_double(), ctypes.c_double()
    cnt = ctypes.c_longlong()
    info = (ctypes.c_longlong * 16)()
    rc = lib().hostlogic_calibrate(_dp(s), _dp(costs), gamma, n, int(target), total, int(max_iter),
                                   int(spec_depth), int(force_exact),
                                   sol.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(pen),
                                   ctypes.byref(val), ctypes.byref(cnt), info)
    assert rc == 0, rc
    keys = ["path", "evaluations", "passes", "zone_iters", "n_diff", "probe_calls", "window_calls",
            "exact_calls", "exact_lambdas", "maps", "spine_calls", "compact_n", "pilot_calls"]
    return pen.value, sol, val.value, cnt.value, dict(zip(keys, [int(x) for x in info]))


def solve_fixed(scores, gamma_or_costs, lam):
    s = np.ascontiguousarray(scores, dtype=np.float64)
    n = s.shape[0]
    if np.isscalar(gamma_or_costs):
        costs, gamma = None, float(gamma_or_costs)
    else:
        costs, gamma = np.ascontiguousarray(gamma_or_costs, dtype=np.float64), 0.0
    sol = np.zeros(n, dtype=np.uint8)
    val = ctypes.c_double()
    cnt = ctypes.c_longlong()
    info = (ctypes.c_longlong * 16)()
    rc = lib().hostlogic_solve_fixed(_dp(s), _dp(costs), gamma, n, float(lam),
                                     sol.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(val),
                                     ctypes.byref(cnt), info)
    assert rc == 0, rc
    return sol, val.value, cnt.value, {"path": int(info[0]), "n_diff": int(info[4])}


MODEL_CHAIN_DEVICE_REGIONS = ["tasks", "walk", "wcap", "state", "points", "results", "ctl", "globals", "writes", "n_writes", "entering", "bits"]
MODEL_CHAIN_FOLLOW_REGIONS = ["report", "n_points", "finals", "facts"]


def model_chain_layout(B, n_wcap, rounds, cap_pairs):
    """The buffers of a chain of rounding-model rounds as csrc/lean_tasks.h lays them out: per buffer a list of
    (region, offset, bytes the region must hold) in the documented order, the totals, and the product's limits."""
    limits = (ctypes.c_int * 4)()
    dev_off, dev_need = (ctypes.c_longlong * 12)(), (ctypes.c_longlong * 12)()
    fol_off, fol_need = (ctypes.c_longlong * 4)(), (ctypes.c_longlong * 4)()
    totals = (ctypes.c_longlong * 3)()
    lib().hostlogic_model_chain_layout(int(B), int(n_wcap), int(rounds), int(cap_pairs), limits, dev_off, dev_need, fol_off, fol_need, totals)
    return {
        "device": list(zip(MODEL_CHAIN_DEVICE_REGIONS, dev_off, dev_need)),
        "follow": list(zip(MODEL_CHAIN_FOLLOW_REGIONS, fol_off, fol_need)),
        "device_bytes": totals[0], "upload_bytes": totals[1], "follow_bytes": totals[2],
        "limits": dict(zip(["chain_max_problems", "model_chain_max_problems", "model_chain_max_rounds", "lean_max_points"], limits)),
    }


RECORD_LAYOUT_REGIONS = {
    "count": ["tracks", "chunk_first", "tile_first", "maxima", "tile_sums", "delta"],
    "interval": ["rec_offsets", "facts", "cand_lo", "cand_n", "units", "unit_first", "scan"],
    "flag_facts": ["rec_offsets", "mapped", "unsorted"],
    "centers": ["raw", "prefix", "density", "index", "density_sorted", "index_sorted", "cub"],
    "xcorr": ["rec_offsets", "min_lag", "block_track", "block_start", "best_lag", "fwd_sum", "rev_sum", "best_score"],
    "template": ["rec_offsets", "min_insert", "counts", "select"],
}


def record_layout(kind, *shape):
    """The scratch buffer of one record launcher as csrc/record_layouts.h lays it out (``kind``: a key of
    `RECORD_LAYOUT_REGIONS`; ``shape``: the integers its layout function takes, for "count" the tracks and the bins of each):
    a list of (region, offset, bytes the region must hold) in the documented order, and the total."""
    names = RECORD_LAYOUT_REGIONS[kind]
    off, need = (ctypes.c_longlong * len(names))(), (ctypes.c_longlong * len(names))()
    total = ctypes.c_longlong()
    getattr(lib(), f"hostlogic_{kind}_layout")(*[ctypes.c_longlong(int(v)) for v in shape], off, need, ctypes.byref(total))
    return list(zip(names, off, need)), total.value
