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


# ---- tests/test_gpu_dispersion_shapes.py: signed matrices with adversarial columns ---------------------------------------

NETWORK_SIZES = (2, 4, 8, 12, 16, 24, 32, 48, 64, 80, 100)  # the KP of dispatch() in rocco_amd/csrc/dispersion.hip
# every network size exactly, and the lowest and the highest padded K of every range
SHAPE_KS = (2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 99, 100)
SHAPE_N = 515  # two full workgroups of 256 lanes and one of three
SHAPE_RNGS = ((25, 75), (0, 100), (12.5, 87.5))
LONG_KS = (101, 128, 129, 264, 968, 969, 1000, 1023, 1024)  # the memory path; 969 and 1023 need the fourth level of the pairwise order


def network_size(K):
    """The register network a column of K <= 100 rows is padded to."""
    return min(kp for kp in NETWORK_SIZES if kp >= K)


def adversarial_columns(K, dtype, gen):
    """[(name, column of K float64 values)] -- the columns a kernel that is right on random positive data can still get
    wrong.  `dtype` "f32": the float32 analogue where the values would not survive the narrowing, or no column."""
    f64 = dtype == "f64"
    huge, tiny = (1.5e308, 1e-310) if f64 else (3.0e38, 1e-42)
    rows = np.arange(K)
    plain = lambda: np.round(2.0 * gen.standard_normal(K), 1)  # noqa: E731
    cols = []
    # zeros of both signs (they compare equal; the sign of a zero answer is still NumPy's)
    cols.append(("all -0.0", np.full(K, -0.0)))
    cols.append(("-0.0 +0.0 in turn", np.where(rows % 2 == 0, -0.0, 0.0)))
    cols.append(("+0.0 -0.0 in turn", np.where(rows % 2 == 0, 0.0, -0.0)))
    cols.append(("zeros among +-1 +-2", np.resize(np.array([-0.0, 1.0, 0.0, -1.0, 2.0, -0.0, -2.0, 0.0]), K)))
    # the orders a wrong comparator of the network survives on random data
    ramp = np.round((rows - (K - 1) / 2.0) * 0.3 + 0.05, 2)  # strictly ascending, both signs
    cols.append(("ascending", ramp))
    cols.append(("descending", ramp[::-1].copy()))
    cols.append(("organ pipe", np.concatenate([ramp[0::2], ramp[1::2][::-1]])))
    for row in sorted({0, K // 2, K - 1}):
        c = np.full(K, 0.7)
        c[row] = -3.3
        cols.append((f"one outlier at row {row}", c))
    for first in sorted({min(max(r + 1, 1), K - 1) for r in (K // 2 - 1, K // 2, K // 2 + 1)}):
        cols.append((f"two values, {first} rows of the first", np.where(rows < first, -1.5, 2.5)))
    # infinities on both sides of MAD's balanced padding: n_lo of the KP - K padding entries are -inf
    n_lo = (network_size(K) - K) // 2 if K <= NETWORK_SIZES[-1] else 0
    counts = sorted({c for c in (1, n_lo, n_lo + 1, (K + 1) // 2 - 1, K // 2 + 1) if 1 <= c <= K})
    for c in counts:
        for name, value in ((f"{c} x -inf", -np.inf), (f"{c} x +inf", np.inf)):
            col = plain()
            col[gen.choice(K, size=c, replace=False)] = value
            cols.append((name, col))
    for c in counts:
        if 2 * c <= K:  # (no column holds more than K entries)
            col = plain()
            where = gen.choice(K, size=2 * c, replace=False)
            col[where[:c]], col[where[c:]] = -np.inf, np.inf
            cols.append((f"{c} x -inf and {c} x +inf", col))
    # finite entries whose sums overflow: in NumPy's pairwise order one accumulator reaches +inf and its neighbour -inf
    cols.append(("+-huge in turn", np.where(rows % 2 == 0, huge, -huge)))
    if f64:
        cols += huge_throughout(K)
    # subnormals: the squared deviations underflow to 0
    cols.append(("subnormal", gen.standard_normal(K) * tiny))
    if f64:  # cancellation in the two-pass variance
        cols.append(("1e15 + small integers", 1e15 + gen.integers(-3, 4, size=K).astype(float)))
    return cols


def huge_throughout(K):
    """1.5e308 in every row but one: for even K the sum of the two middle values overflows and the MEDIAN is +inf, with every
    entry finite.  SciPy's MAD is then +inf (every deviation is), NaN only where an entry is +inf itself (inf - inf)."""
    c = np.full(K, 1.5e308)
    c[K // 3] = 1.0e308
    cols = [("huge throughout", c)]
    if K >= 4:  # (in shorter columns the infinity would be one of the middle values)
        for name, value in (("huge throughout and one +inf", np.inf), ("huge throughout and one -inf", -np.inf)):
            c = c.copy()
            c[K - 1] = value
            cols.append((name, c))
    return cols


def signed_matrix(K, n, dtype, adversarial=True):
    """(K x n matrix, [column names]): np.round(2 * standard_normal, 1) -- both signs, many ties, now and then a -0.0 --
    with column 0 the constant -1.25 and column 1 holding one NaN; from column 2 on `adversarial_columns`, one plain column
    between each two (as far as n reaches)."""
    gen = np.random.default_rng([K, n, 41 if dtype == "f32" else 40])
    with np.errstate(all="ignore"):
        m = np.round(2.0 * gen.standard_normal((K, n)), 1)
        names = ["plain"] * n
        m[:, 0], names[0] = -1.25, "constant"
        if n >= 2:
            m[int(gen.integers(0, K)), 1], names[1] = np.nan, "one NaN"
        if adversarial:
            for i, (name, column) in enumerate(adversarial_columns(K, dtype, gen)):
                if 2 + 2 * i < n:
                    m[:, 2 + 2 * i], names[2 + 2 * i] = column, name
        return (m.astype(np.float32) if dtype == "f32" else m), names


LONG_N = 68


def long_matrix(K):
    """The matrix of the K > 100 cases: 64 signed columns, the overflowing one (column 64) and `huge_throughout`."""
    m, names = signed_matrix(K, 64, "f64", adversarial=False)
    extra = [("+-huge in turn", np.where(np.arange(K) % 2 == 0, 1.5e308, -1.5e308))] + huge_throughout(K)
    return np.concatenate([m] + [column[:, None] for _, column in extra], axis=1), names + [name for name, _ in extra]


def both_zeros(m):
    """Per column: whether it holds a -0.0 and a +0.0."""
    zero, negative = (m == 0), np.signbit(m)
    return (zero & negative).any(axis=0) & (zero & ~negative).any(axis=0)


def trimmed_columns(job):
    """(kind, K, n, dtype, tprop, root) -> per column stats.tstd (root) or stats.tvar (not root) between the
    np.quantile(..., method="nearest") limits at tprop and 1 - tprop; kind "signed": signed_matrix, "long": long_matrix."""
    from scipy import stats

    kind, K, n, dtype, tprop, root = job
    m = np.asarray(signed_matrix(K, n, dtype)[0] if kind == "signed" else long_matrix(K)[0], dtype=float)
    fn = stats.tstd if root else stats.tvar
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        lo = np.quantile(m, tprop, axis=0, method="nearest")
        hi = np.quantile(m, 1.0 - tprop, axis=0, method="nearest")
        return np.array([fn(m[:, j], limits=(lo[j], hi[j]), inclusive=(True, True)) for j in range(m.shape[1])], dtype=float)


def trimmed_expected(jobs):
    """`trimmed_columns` of every job, 16 worker processes at the most."""
    procs = max(1, min(16, len(jobs), len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16))
    if procs == 1:
        return [trimmed_columns(j) for j in jobs]
    with mp.get_context("spawn").Pool(procs) as pool:
        return pool.map(trimmed_columns, jobs, chunksize=1)
