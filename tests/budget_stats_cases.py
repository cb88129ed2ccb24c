"""What tests/test_gpu_budget_stats.py, tests/test_budget_stats_cases_host.py and tests/golden/make_golden_budget_long_lag.py
share: inputs and expected values for the kernels of rocco_amd/csrc/budget_stats.hip (radix sort of doubles, sorted probe,
autocovariance sums, negative part, soft counts).

Autocovariance sums are pinned two ways.  EXACT cases: x integer-valued in [-512, 512], `mean` an integer or a half-integer,
so every x - mean is a multiple of 1/2, every product a multiple of 1/4 below 2^21 / 4 and every partial sum a multiple of
1/4 below 2^35 / 4: all of them are float64 numbers, no rounding happens in any summation order, with or without fused
multiply-add, and the result must equal the integer dot product bit for bit.  REAL cases: the expected value is the exact
rational sum of the products of c = x - mean (c rounded once, as the kernel rounds it), and the distance allowed is the
textbook bound of a sequential sum, see `real_bound`.

The sort's order is that of the bit patterns (`sort_key`): sign-set NaNs, -inf, negative values, -0.0, +0.0, positive
values, +inf, sign-clear NaNs; ties keep nothing to tell apart (equal keys are equal bit patterns).

NumPy only: imported by a host test, by GPU tests and by the golden generator alike."""
import functools
from fractions import Fraction

import numpy as np

SEG = 4096        # loci per workgroup of the autocovariance kernel
CHUNK = 1024      # lags per launch
U = Fraction(1, 2 ** 53)
NEG_NAN = np.copysign(np.nan, -1.0)

# ------------------------------------------------------------------------------------------------------------------
# B1: exact autocovariance sums
# ------------------------------------------------------------------------------------------------------------------
EXACT_LENGTHS = (1, 2, 5, 4095, 4096, 4097, 5119, 5120, 8192, 8193, 12289, 16385)
EXACT_MAX_LAGS = (0, 1, 2, 255, 256, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5119)
EXACT_MEANS = (0.0, 7.0, -2.5)  # doubled: 0, 14, -5
SPIKE_N = 12289
SPIKE_POSITIONS = (0, 4095, 4096, 8191, None)  # None: n - 1 - k
SPIKE_LAGS = (1, 1023, 1024, 1025, 4096, 4097)
SPIKE_MAX_LAG = 5119
SPIKE_VALUES = (-371.0, 509.0)
SPIKE_MEANS = (0.0, 1.5)


def max_lags_for(n):
    """The issue's lag caps and n - 1, each capped at n - 1, duplicates dropped, ascending."""
    return sorted({min(k, n - 1) for k in EXACT_MAX_LAGS + (n - 1,)})


def exact_track(n, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    x = rng.integers(-512, 513, size=n).astype(np.float64)
    if n >= 2:
        x[0], x[-1] = 512.0, -512.0  # the extremes are present, and at the ends where a lost term shows
    return x


def spike_track(n, p, k, a=SPIKE_VALUES[0], b=SPIKE_VALUES[1]):
    x = np.zeros(n, dtype=np.float64)
    x[p], x[p + k] = a, b
    return x


def spike_cases():
    """(p, k) of every two-spike track of length SPIKE_N."""
    cases = []
    for k in SPIKE_LAGS:
        for p in SPIKE_POSITIONS:
            p = SPIKE_N - 1 - k if p is None else p
            if (p, k) not in cases:
                cases.append((p, k))
    return cases


def exact_sums(x, mean, max_lag):
    """sum_i (x_i - mean)(x_{i+k} - mean) for k = 0..max_lag in integer arithmetic (x integer-valued, 2 mean an integer)."""
    xi, m2 = np.asarray(x).astype(np.int64), int(round(2 * mean))
    assert np.array_equal(xi.astype(np.float64), x) and m2 == 2 * mean
    d = 2 * xi - m2
    n = d.size
    sums = np.array([int(np.dot(d[:n - k], d[k:])) for k in range(max_lag + 1)], dtype=np.int64)
    assert np.all(sums % 1 == 0) and np.all(np.abs(sums) < 2 ** 53)
    return sums.astype(np.float64) / 4.0


@functools.lru_cache(maxsize=None)
def exact_sums_all_lags(n, mean):
    """exact_sums of exact_track(n) at every lag 0..n-1 (computed once; a test slices it)."""
    out = exact_sums(exact_track(n), mean, n - 1)
    out.setflags(write=False)
    return out


def spike_sums(n, p, k, mean, max_lag, a=SPIKE_VALUES[0], b=SPIKE_VALUES[1]):
    """exact_sums of spike_track(n, p, k) in closed form: sum x_i x_{i+j} is a b at j = k, a^2 + b^2 at j = 0 and 0 elsewhere;
    sum (x_i - m)(x_{i+j} - m) = sum x_i x_{i+j} - m (sum of the first n - j values + sum of the last n - j) + (n - j) m^2,
    all in integers of doubled values (tests/test_budget_stats_cases_host.py holds it against exact_sums)."""
    x = spike_track(n, p, k, a, b).astype(np.int64)
    m2 = int(round(2 * mean))
    prefix = np.concatenate([[0], np.cumsum(x)])
    j = np.arange(max_lag + 1)
    products = np.zeros(max_lag + 1, dtype=np.int64)
    products[0] = int(a * a + b * b)
    products[k] += int(a * b)
    heads, tails = prefix[n - j], prefix[n] - prefix[j]
    sums = 4 * products - 2 * m2 * (heads + tails) + (n - j) * m2 * m2
    return sums.astype(np.float64) / 4.0


def exactness_bound(n_max, x_abs_max, mean_abs_max):
    """Largest |4 x partial sum| any exact case can reach: n terms of (2|x| + 2|mean|)^2."""
    return n_max * (2 * x_abs_max + int(round(2 * mean_abs_max))) ** 2


# ------------------------------------------------------------------------------------------------------------------
# B2: real-valued autocovariance sums
# ------------------------------------------------------------------------------------------------------------------
REAL_LENGTHS = (8193, 12289)
REAL_LAGS = (0, 1, 2, 1023, 1024, 1025, 2048, 4096, 4097, None)  # None: n - 1


def real_track(kind, n):
    rng = np.random.default_rng(77 + n)
    if kind == "gamma":  # soft counts of a gamma background over a 1e-6 scale, as the estimate makes them
        return np.clip(np.round(rng.gamma(1.0, 0.3, size=n), 5) - 0.21, 0.0, None) / 0.3127
    return np.linspace(-0.5, 3.0, n) + 0.3 * rng.normal(size=n)  # "ramp": long positive autocorrelation, both signs


def real_lags(n):
    return [n - 1 if k is None else k for k in REAL_LAGS]


def real_reference(x, mean, lags):
    """{lag: (exact rational sum of c_i c_{i+k}, exact sum of |c_i c_{i+k}|)}, c = float64(x - mean)."""
    c = np.asarray(x, dtype=np.float64) - np.float64(mean)
    f = [Fraction(float(v)) for v in c]
    n = len(f)
    out = {}
    for k in lags:
        total, absolute = Fraction(0), Fraction(0)
        for i in range(n - k):
            p = f[i] * f[i + k]
            total += p
            absolute += abs(p)
        out[k] = (total, absolute)
    return out


def real_bound(n, absolute):
    """gamma_m x sum |c_i c_{i+k}|, m = 4096 + B + 1 with B the number of 4096-locus segments: a lane adds at most 4096
    rounded products in order (m' = 4096 operations with FMA contraction, 4096 + 1 without), the B partial sums are then
    added in order (B more).  gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and Stability, section 3.1)."""
    m = SEG + (n + SEG - 1) // SEG + 1
    return (m * U) / (1 - m * U) * absolute


# ------------------------------------------------------------------------------------------------------------------
# C: long-lag tracks for the truncation lag / effective sample size
# ------------------------------------------------------------------------------------------------------------------
RAMP_LENGTHS = (8193, 12289, 16385)
ESTIMATE_HINTS = (256, 300, 2000)
PAIR_MARGIN = 1.0e-6


def ramp_track(n):
    rng = np.random.default_rng(n)
    return np.round(np.clip(np.linspace(-0.5, 3.0, n) + 0.3 * rng.normal(size=n), 0.0, None), 5)


def ess_max_lags(n):
    return [1023, 1024, 1025, 2049, 5000, n - 1]


def wanted_lags_above(n, max_lag):
    """A stored case with this lag cap must use MORE lags than this: caps up to 2049 must be used up (cap - 1), the caps
    beyond must pass two lag chunks (n = 8193) or four, i.e. the segment length (the longer tracks)."""
    cap = int(min(max(2, max_lag), n - 1))
    if cap <= 2049:
        return cap - 1
    return 2048 if n <= 8193 else 4096


def soft_counts(scores, center, scale):
    return np.clip(np.asarray(scores, dtype=np.float64) - center, 0.0, None) / max(scale, 1.0e-6)


def geyer_pairs(values, max_lag):
    """Geyer's pair sums of the autocorrelations from direct lagged-product sums: (pairs met, up to and including the one
    that ends the sum or the last one under the cap; lags used; tau)."""
    v = np.asarray(values, dtype=np.float64)
    n = v.size
    c = v - float(np.mean(v))
    cap = int(min(max(2, max_lag), n - 1))
    acov = np.correlate(c, c, mode="full")[n - 1:n + cap] / np.arange(n, n - cap - 1, -1, dtype=np.float64)
    acf = np.clip(acov[1:] / acov[0], -1.0, 1.0)
    tau, used, pairs = 1.0, 0, []
    for k in range(0, acf.size, 2):
        pair = float(acf[k]) + (float(acf[k + 1]) if k + 1 < acf.size else 0.0)
        pairs.append(pair)
        if not np.isfinite(pair) or pair <= 0.0:
            break
        tau += 2.0 * pair
        used = int(min(cap, k + 2))
    return np.array(pairs), used, tau


# ------------------------------------------------------------------------------------------------------------------
# E: tracks with non-finite values
# ------------------------------------------------------------------------------------------------------------------
BAD_VALUES = {"nan": np.nan, "negnan": NEG_NAN, "posinf": np.inf, "neginf": -np.inf}
NONFINITE_ESS_MAX_LAG = 404


def signal_track(n=4000, seed=2):
    """The "signal" track of tests/golden/make_golden_budget.py."""
    rng = np.random.default_rng(seed)
    s = np.round(rng.gamma(1.0, 0.3, size=n), 5)
    for p in rng.integers(0, n, size=max(1, n // 400)):
        s[p:p + int(rng.integers(4, 40))] += rng.gamma(6.0, 1.0)
    return np.round(s, 5)


def short_track():
    return np.array([-0.75, 0.5, 1.25])


def nonfinite_tracks():
    """[(name, track)]: one bad value at index 0, the middle and n - 1 of the 4000-long signal track and of a 3-long
    track; a track with 10 % NaNs; an all-NaN track.  Names: <bad>_<track>_<position>, bad in BAD_VALUES."""
    out = []
    for bad, value in BAD_VALUES.items():
        for label, base in (("signal", signal_track()), ("short", short_track())):
            for where, at in (("first", 0), ("middle", base.size // 2), ("last", base.size - 1)):
                s = base.copy()
                s[at] = value
                out.append((f"{bad}_{label}_{where}", s))
    s = signal_track()
    s[np.random.default_rng(5).permutation(s.size)[:s.size // 10]] = np.nan
    out.append(("nan_signal_tenth", s))
    out.append(("nan_signal_all", np.full(4000, np.nan)))
    return out


def bad_class(name):
    return name.split("_")[0]


# ------------------------------------------------------------------------------------------------------------------
# D1: the sort
# ------------------------------------------------------------------------------------------------------------------
SORT_LENGTHS = (1, 2, 3, 255, 256, 257, 4096, 65537)
SORT_KINDS = ("bits", "specials", "one-value", "sixteen-values")
SPECIAL_BITS = np.array([
    0x0000000000000000, 0x8000000000000000,                      # +0.0, -0.0
    0x7FF0000000000000, 0xFFF0000000000000,                      # +inf, -inf
    0x0000000000000001, 0x8000000000000001,                      # smallest denormals
    0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,                      # largest denormals
    0x0010000000000000, 0x8010000000000000,                      # smallest normals
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,                      # largest normals
    0x7FF8000000000000, 0xFFF8000000000000,                      # the default quiet NaN, either sign
    0x7FF0000000000001, 0xFFF0000000000001,                      # signalling NaNs, smallest payload
    0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,                      # NaNs, largest payload
    0x7FF8000000ABCDEF, 0xFFF4000000123456,                      # NaNs with payloads in the middle
    0x3FF0000000000000, 0xBFF0000000000000,                      # 1.0, -1.0
], dtype=np.uint64)


def sort_key(bits):
    """Order-preserving key of a float64 bit pattern: all bits flipped when the sign is set, else the sign bit set."""
    bits = np.asarray(bits, dtype=np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))


def expected_sorted_bits(bits):
    bits = np.asarray(bits, dtype=np.uint64)
    return bits[np.argsort(sort_key(bits), kind="stable")]


def sort_input_bits(kind, n):
    """uint64 bit patterns of the n doubles to sort."""
    rng = np.random.default_rng(31 * n + SORT_KINDS.index(kind))
    if kind == "bits":
        return rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    if kind == "specials":  # every special value (several times where n allows), the rest random finite values, shuffled
        bits = rng.normal(size=n).view(np.uint64).copy()
        reps = np.tile(SPECIAL_BITS, max(1, min(3, n // SPECIAL_BITS.size)))
        reps = reps[rng.permutation(reps.size)][:n]  # (n below the list's length: a random part of it)
        bits[rng.permutation(n)[:reps.size]] = reps
        return bits
    if kind == "one-value":
        return np.full(n, np.float64(-2.625).view(np.uint64), dtype=np.uint64)
    values = np.concatenate([SPECIAL_BITS[:6], rng.normal(size=10).view(np.uint64)])  # 16 distinct values, heavy ties
    return values[rng.integers(0, 16, size=n)]


# ------------------------------------------------------------------------------------------------------------------
# D2: the probe
# ------------------------------------------------------------------------------------------------------------------
MERGE_SHIFT = 1.0 - 2.0 ** -30


def merging_case():
    """(sorted x, shift) for which x - shift rounds distinct neighbours to one double: x_j = 2^30 + j 2^-22 (one unit in
    the last place of 2^30 apart), shift = -(2^31 + 2^30), so x - shift = 2^32 + j 2^-22 where float64 is 2^-20 apart:
    about four neighbouring x share a difference.  (A subtraction merges only when the difference is LARGER than x.)"""
    j = np.arange(64, dtype=np.float64)
    return 2.0 ** 30 + j * 2.0 ** -22, -(2.0 ** 31 + 2.0 ** 30)


def cancelling_case():
    """(sorted x, shift) with x_j = 1 + j 2^-52 and shift = 1 - 2^-30: the subtraction cancels 30 leading bits and is
    exact (Sterbenz), so NO neighbours merge -- kept as the opposite case: thresholds one unit apart must count apart."""
    j = np.arange(64, dtype=np.float64)
    return 1.0 + j * 2.0 ** -52, MERGE_SHIFT


def tie_vector():
    """Sorted: values occurring 1, 2 and 1000 times among 300 others, -0.0 and +0.0 side by side, both infinities."""
    rng = np.random.default_rng(12)
    others = np.round(rng.normal(size=300), 3) + 1.0e-4  # (no multiple of 1e-3: none of the tied values below)
    body = np.concatenate([others, [0.5], [1.75, 1.75], np.full(1000, -1.125), [-0.0, 0.0, 0.0, -0.0], [-np.inf, np.inf, np.inf]])
    return expected_sorted_bits(body.view(np.uint64)).view(np.float64).copy()


def probe_vectors():
    """{name: sorted float64 vector without NaN}"""
    rng = np.random.default_rng(13)
    big = np.sort(np.round(rng.normal(size=70001), 2))  # n above 2^16, heavy ties
    return {"ties": tie_vector(), "one": np.array([3.5]), "two": np.array([-2.0, 7.25]), "big": big,
            "merge": merging_case()[0], "cancel": cancelling_case()[0]}


def probe_thresholds(x):
    """Thresholds at, between, below and above the values of a sorted vector, the infinities and zero (at most 8 a call:
    the caller chunks them)."""
    finite = x[np.isfinite(x)]
    values, counts = np.unique(finite, return_counts=True)
    picks = [values[0], values[-1], values[np.argmax(counts)], values[np.argmin(counts)], values[values.size // 2]]
    picks += list(values[counts == 2][-1:])  # a value that occurs exactly twice, where there is one
    between = [(values[i] + values[i + 1]) / 2.0 for i in (0, values.size // 2 - 1, values.size - 2) if 0 <= i < values.size - 1]
    outside = [np.nextafter(values[0], -np.inf), values[0] - 1.0, np.nextafter(values[-1], np.inf), values[-1] + 1.0]
    return [float(t) for t in picks + between + outside + [np.inf, -np.inf, 0.0, -0.0]]


def probe_counts(x, shift, thresholds):
    v = x - np.float64(shift)
    return [int((v <= t).sum()) for t in thresholds], [int((v < t).sum()) for t in thresholds]


# ------------------------------------------------------------------------------------------------------------------
# D3: elementwise helpers
# ------------------------------------------------------------------------------------------------------------------
ELEMENTWISE_LENGTHS = (1, 255, 256, 257, 8193)
CENTER, SCALE = 0.1234567890123457, 0.9876543210987654  # long mantissas


def elementwise_input(n):
    rng = np.random.default_rng(40 + n)
    v = rng.normal(size=n)
    specials = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, CENTER,
                         np.nextafter(CENTER, 1.0), np.nextafter(CENTER, -1.0), 1e300, -1e300])
    at = rng.permutation(n)[:min(n, specials.size)]
    v[at] = specials[rng.permutation(specials.size)[:at.size]]
    if n == 1:
        v[0] = CENTER
    return v


def negative_part(v):
    return v - np.clip(v, 0.0, None)


def soft(v, c, s):
    return np.clip(v - c, 0.0, None) / s
