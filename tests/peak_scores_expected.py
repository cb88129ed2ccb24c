"""Test helper: the post-hoc peak scoring (rocco/scores.py:120-149, 176-192, 583) restated in NumPy / SciPy calls, and the
deterministic inputs that tests/test_peak_scores_host.py, tests/test_gpu_peak_scores.py and
tests/golden/make_golden_scores.py share.  Nothing here imports the package under test.  TEST INFRASTRUCTURE ONLY."""
import functools
import warnings

import numpy as np

from log2_truth import log2_correctly_rounded

PS = (1, 255, 256, 257, 1000)                    # the block edges of the one-lane-per-peak kernels (256 lanes)
KS = (1, 2, 3, 4, 5, 7, 8, 12, 33, 100)
KINDS = ("integer", "continuous", "mostly_zero", "with_inf", "with_nan")
LENGTHS = (0.0, 0.4, 1.0, 250.9, -3.0, 4000.0)   # int() of them: 0, 0, 1, 250, -3, 4000 -> max(..., 1)
PERCENTILES = (0, 0.1, 5, 10, 33.3, 50, 75, 90, 95, 99.9, 100)
PCS = (0.0, 0.5, 1.0, 2.0)
ROW_SCALES = (1.0, 1000.0, 1e6)
# where `n q + (1 - q) - 1` and `(n - 1) q` cannot differ: q = 0 and q = 1 are exact in both, q = 0.5 and q = 0.75 are
# exact in both while n < 2^51.  Every other percentile of the list has a K in KS at which the two round apart.
RANK_RULES_AGREE_AT = (0, 50, 75, 100)
BH_SIZES = (1, 2, 3, 1023, 1024, 1025)
BH_INVALID = (float("nan"), -1e-300, 1.0 + 2.0 ** -52)
BH_ERROR = "`ps` must include only numbers between 0 and 1."


def quiet(function):
    """log2(0), inf - inf and NaN comparisons are what these inputs are for: no RuntimeWarning for them."""
    @functools.wraps(function)
    def wrapped(*args, **kwargs):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            return function(*args, **kwargs)
    return wrapped


# ---- the restatement ---------------------------------------------------------------------------------------------------

def log2_exact(t):
    """The correctly rounded log2 where the argument is finite and positive, np.log2 (-inf, inf, NaN) everywhere else."""
    t = np.asarray(t, dtype=np.float64)
    regular = np.isfinite(t) & (t > 0.0)
    with np.errstate(all="ignore"):
        out = np.log2(t)
    if regular.any():
        out[regular] = log2_correctly_rounded(t[regular])
    return out


@quiet
def transformed(counts, lengths, row_scale, pc, log2=log2_exact):
    """log2(np.maximum(vals * (row_scale / max(int(length), 1)) + pc, pc)) of every row (rocco/scores.py:184-191)."""
    counts = np.asarray(counts, dtype=np.float64)
    length_ = np.array([float(max(int(length), 1)) for length in np.asarray(lengths, dtype=np.float64)])
    return log2(np.maximum(counts * (float(row_scale) / length_)[:, None] + float(pc), float(pc)))


@quiet
def signal(counts, lengths, row_scale, pc, percentile, log2=log2_exact):
    """`_peak_signal_stat` of every row of a [peaks, samples] matrix; `percentile` a number (-> [peaks]) or a sequence
    (-> [len(percentile), peaks], np.percentile's own layout; the same values as one call per entry)."""
    return np.percentile(transformed(counts, lengths, row_scale, pc, log2), percentile, axis=1)


def survival(stat, bins, nulls):
    """`EmpiricalNull(nulls[bins[i]]).survival(stat[i])` (rocco/scores.py:128-141), `nulls` a mapping key -> values."""
    out = np.empty(len(stat), dtype=np.float64)
    for i, (x, b) in enumerate(zip(np.asarray(stat, dtype=np.float64), bins)):
        values = np.sort(np.asarray(nulls[int(b)], dtype=np.float64))
        out[i] = (values.size - np.searchsorted(values, x, side="left") + 1.0) / (values.size + 1.0)
    return out


def bh(p):
    from scipy import stats

    return np.atleast_1d(stats.false_discovery_control(np.asarray(p, dtype=np.float64), method="bh"))


def same_values(got, want) -> bool:
    """Equal bits wherever `want` is finite, a NaN where it is NaN, the same infinity where it is infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes())


# ---- the two rank rules, in float64 scalars (host test only: which inputs can tell them apart) --------------------------

def virtual_index_numpy(K, percentile):
    """NumPy's `linear`: (n - 1) * quantiles."""
    return np.float64(K - 1) * (np.float64(percentile) / np.float64(100.0))


def virtual_index_general(K, percentile):
    """The general form of the other methods at alpha = beta = 1: n q + (1 - q) - 1."""
    q = np.float64(percentile) / np.float64(100.0)
    return np.float64(K) * q + (np.float64(1.0) - q) - np.float64(1.0)


def brackets(K, vi):
    """(previous, next, gamma) as NumPy's _get_indexes / _get_gamma leave them for a virtual index in [0, K - 1]."""
    prev = int(np.floor(vi))
    gamma = np.float64(vi) - np.float64(prev)
    return min(max(prev, 0), K - 1), min(max(prev + 1, 0), K - 1), gamma


@quiet
def lerp_rows(ordered, prev, nxt, gamma):
    """NumPy's _lerp between two columns of row-sorted values."""
    a, b = ordered[:, prev], ordered[:, nxt]
    diff = b - a
    return b - diff * (np.float64(1.0) - gamma) if gamma >= 0.5 else a + diff * gamma


# ---- the cases ---------------------------------------------------------------------------------------------------------

def shape_cases():
    """Every (P, K) of PS x KS once; the kind rotates so that each kind meets every K and every P."""
    return [dict(index=ip * len(KS) + ik, P=P, K=K, kind=KINDS[(ip + ik) % len(KINDS)])
            for ip, P in enumerate(PS) for ik, K in enumerate(KS)]


def parameters(case):
    """The (pc, row_scale) pairs of a case: every pc, the row scale rotating with K (so each kind meets all twelve)."""
    return [(pc, ROW_SCALES[(KS.index(case["K"]) + j) % len(ROW_SCALES)]) for j, pc in enumerate(PCS)]


@functools.lru_cache(maxsize=None)
def _inputs(index):
    case = shape_cases()[index]
    P, K, kind = case["P"], case["K"], case["kind"]
    gen = np.random.default_rng([index, P, K, 4])
    lengths = np.asarray(LENGTHS)[(np.arange(P) + index) % len(LENGTHS)].copy()
    plain = gen.random(P) < 0.3
    lengths[plain] = gen.integers(50, 4000, size=int(plain.sum())).astype(np.float64)
    if kind == "integer":
        counts = gen.integers(0, 4, size=(P, K)).astype(np.float64)  # 4 values over K samples: ties at every rank
    elif kind == "mostly_zero":
        counts = gen.integers(1, 6, size=(P, K)).astype(np.float64)
        for row in counts:
            zeros = int(gen.integers(int(np.ceil(0.6 * K)), K + 1))
            row[gen.permutation(K)[:zeros]] = 0.0
    else:
        counts = gen.gamma(2.0, 30.0, size=(P, K)) * (np.maximum(lengths, 1.0)[:, None] / 500.0)
        counts[gen.random((P, K)) < 0.05] = 0.0
        rows = np.flatnonzero(gen.random(P) < 0.4)
        if rows.size == 0:
            rows = np.array([0])
        for r in rows:
            if kind == "with_inf":
                spots = gen.permutation(K)
                which = int(gen.integers(0, 3))  # +inf, -inf, both
                if which != 1:
                    counts[r, spots[0]] = np.inf
                if which != 0:
                    counts[r, spots[-1]] = -np.inf
            elif kind == "with_nan":
                counts[r, int(gen.integers(0, K))] = np.nan
    counts.setflags(write=False)
    lengths.setflags(write=False)
    return counts, lengths


def inputs(case):
    """(counts [P, K], lengths [P]) of a case, read-only."""
    return _inputs(case["index"])


@functools.lru_cache(maxsize=None)
def _expected(index, pc, row_scale):
    counts, lengths = _inputs(index)
    out = signal(counts, lengths, row_scale, pc, PERCENTILES)
    out.setflags(write=False)
    return out


def expected_signal(case, pc, row_scale):
    """[len(PERCENTILES), P]: the restatement with the correctly rounded logarithm; computed once, read-only."""
    return _expected(case["index"], float(pc), float(row_scale))


# the part of the cases that tests/golden/make_golden_scores.py records from the reference (K <= 33, P <= 257; every
# kind twice, every percentile, pc and row scale; the first FIXTURE_ROWS rows of a case)
FIXTURE_CASES = (0, 2, 4, 8, 11, 15, 21, 28, 36, 38)
FIXTURE_ROWS = 40


def survival_cases():
    """[(name, null values as handed over (unsorted), statistics)]: nulls of size 1, 2 and a few hundred, statistics that
    are NaN, +-inf, below and above every null value, and exactly on null values (repeated ones among them)."""
    gen = np.random.default_rng(404)
    big = np.round(gen.gamma(2.0, 1.2, size=307), 1)  # one decimal: most values repeat
    edges = [np.nan, np.inf, -np.inf, -1.0, 1e9]
    with_inf = np.concatenate([np.round(gen.normal(size=200), 1), [-np.inf] * 7, [np.inf] * 2])
    with_nan = np.concatenate([np.round(gen.normal(size=50), 1), [-np.inf, -np.inf, np.nan, np.nan]])
    return [
        ("one", np.array([2.0]), np.array(edges + [2.0, np.nextafter(2.0, 3.0), np.nextafter(2.0, 1.0)])),
        ("two", np.array([3.5, -0.25]), np.array(edges + [3.5, -0.25, 0.0, 3.4999])),
        ("two_equal", np.array([2.0, 2.0]), np.array(edges + [2.0, 1.0, 3.0])),
        ("hundreds", big, np.concatenate([edges, big[:60], gen.gamma(2.0, 1.2, size=40), [big.min(), big.max()]])),
        ("hundreds_with_inf", with_inf, np.concatenate([edges, with_inf[:40], [-1e300, 1e300]])),
        ("with_nan_values", with_nan, np.concatenate([edges, with_nan[:20], [5.0]])),
    ]


def bh_vectors(m):
    """{name: p-values of length m}: many ties, all equal, all 0, all 1, a -0.0 among positive values."""
    gen = np.random.default_rng([m, 9])
    ties = np.round(gen.random(m) ** 2, 1)
    negative_zero = np.maximum(np.round(gen.random(m), 2), 0.01)
    negative_zero[m // 2] = -0.0
    return {"ties": ties, "all_equal": np.full(m, 0.3), "all_zero": np.zeros(m), "all_one": np.ones(m),
            "negative_zero": negative_zero}


def bh_invalid_vectors(m):
    """p-values of length m, valid but for one entry out of BH_INVALID."""
    gen = np.random.default_rng([m, 10])
    out = []
    for bad in BH_INVALID:
        p = gen.random(m)
        p[int(gen.integers(0, m))] = bad
        out.append(p)
    return out
