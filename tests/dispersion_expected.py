"""Test helper: the inputs of tests/test_gpu_dispersion.py and what NumPy / SciPy compute for them.  The per-column
stats.tstd loop (most of a millisecond per column) runs in spawned worker processes: no torch and no GPU in the
children (fork after HIP initialisation is unsafe).  TEST INFRASTRUCTURE ONLY."""
import multiprocessing as mp
import os
import warnings

import numpy as np

KS = (2, 3, 5, 7, 8, 9, 10, 33, 64, 100, 101, 129, 137, 300)
RNGS = ((25, 75), (10, 90), (12.5, 87.5), (0, 100), (33, 66.6), (75, 25), (50, 50), (1, 99))
TPROPS = (0.0, 0.05, 0.2, 0.5)
N = 20011


def matrix(K, n, dtype, with_inf):
    """A fresh K x n matrix with many ties (two decimals); for n >= 2 column 0 is constant and column 1 holds a NaN.
    `with_inf`: +inf, -inf, both, and +inf in more than half of the rows, in columns 2..5 (n >= 6)."""
    gen = np.random.default_rng([K, n, 31 if dtype == "f32" else 30])
    m = np.round(gen.gamma(2.0, 1.5, size=(K, n)), 2)
    if n >= 2:
        m[:, 0] = 1.25
        m[int(gen.integers(0, K)), 1] = np.nan
    if with_inf and n >= 6:
        m[int(gen.integers(0, K)), 2] = np.inf
        m[int(gen.integers(0, K)), 3] = -np.inf
        m[0, 4], m[K - 1, 4] = np.inf, -np.inf
        m[: K // 2 + 1, 5] = np.inf
    return m.astype(np.float32) if dtype == "f32" else m


def tstd_columns(job):
    """(K, n, dtype, tprop) -> the per-column SciPy loop the reference's tmean branch has, for the standard deviation."""
    from scipy import stats

    K, n, dtype, tprop = job
    m = np.asarray(matrix(K, n, dtype, False), dtype=float)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo = np.quantile(m, tprop, axis=0, method="nearest")
        hi = np.quantile(m, 1.0 - tprop, axis=0, method="nearest")
        return np.array([stats.tstd(m[:, j], limits=(lo[j], hi[j]), inclusive=(True, True)) for j in range(n)], dtype=float)


def tstd_expected(jobs):
    """`tstd_columns` of every job, 16 worker processes at the most."""
    procs = max(1, min(16, len(jobs), len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16))
    if procs == 1:
        return [tstd_columns(j) for j in jobs]
    with mp.get_context("spawn").Pool(procs) as pool:
        return pool.map(tstd_columns, jobs, chunksize=1)
