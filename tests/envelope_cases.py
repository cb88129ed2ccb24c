"""Inputs shared by the calibration-envelope tests (tests/test_gpu_calibration_envelope.py on the GPU, the envelope
tests of tests/test_host_logic.py on the CPU): score tracks, the rungs that step across each numeric gate of the fast
path (rocco_amd/csrc/search.cpp: fast_path_applicable, analytic_count, bound_epsilon; the device director's copy in
rocco_amd/csrc/chain.hip), the targets, and the rules both files judge an answer by.

Every rung here returns from the oracle in well under a second: switch costs whose np.sum is not finite and non-finite
scores are NOT among them (the reference's own bisection does not end on the former and rejects the latter)."""
import numpy as np

_KIND_ID = {"peaks": 0, "integers": 1, "normal": 2}

GAMMA_RUNGS = (1e-310, 9.99e-4, 1e-3, 1e6, 1.000001e6, 1e17)
OFFSET_RUNGS = (9e11, -9e11, 1.1e12, 1e15, 1e16, 1e17, 1e18, 1e20, -1e20, 1e300)
SPREAD_RUNGS = ((1e9, 1e-3), (1e9, 1.0), (1e9, 1e6), (1.0000001e9, 1.0))
SIGMA_RUNGS = (1e300, 1e-310)
COMBINED = "combined:offset=9e11,gamma=1e-3"  # the worst case inside every gate at once (budget 0.5)

def widened(rung, n):
    """The rungs on which min - sum(costs) - 1 and max + sum(costs) + 1 round back to min and max (the sum is below
    half a unit in the last place of the scores: 8192 at 1e20), so the reference's bracket is empty and it widens one
    end once: 63 chain evaluations instead of 62 (rocco/dp.py:113-133)."""
    return rung == "offset=1e+300" or (rung in ("offset=1e+20", "offset=-1e+20") and n <= 8193)


LADDER = (["gamma=%r" % g for g in GAMMA_RUNGS] + ["offset=%r" % o for o in OFFSET_RUNGS]
          + ["spread=%r,gamma=%r" % sg for sg in SPREAD_RUNGS] + ["sigma=%r" % s for s in SIGMA_RUNGS] + [COMBINED])
# the rungs that move the magnitude of the scores (the fixed-penalty group walks these)
MAGNITUDE_LADDER = (["offset=0.0"] + ["offset=%r" % o for o in OFFSET_RUNGS] + ["spread=1000000000.0,gamma=1.0"]
                    + ["sigma=%r" % s for s in SIGMA_RUNGS])


def track(kind, n, seed=0):
    """The tracks of tests/test_gpu_chain.py (`peaks`, `integers`, `normal`), seeded by kind, length and `seed`."""
    rng = np.random.default_rng([_KIND_ID[kind], n, seed])
    if kind == "peaks":  # a noise floor with enriched stretches: the shape of the benchmark's tracks
        s = np.round(rng.gamma(1.0, 0.3, n), 5)
        for p in range(50, max(51, n - 50), 1500):
            s[p:p + int(rng.integers(4, 40))] += rng.gamma(6.0, 1.0)
        return s
    if kind == "normal":
        return rng.normal(0.0, 1.0, n)
    return rng.integers(-3, 9, n).astype(np.float64)  # "integers": ties everywhere


def rung_problem(rung, kind, n):
    """(scores, gamma) of one rung: the track of `kind` with ONE gate's quantity moved, everything else ordinary."""
    t = track(kind, n)
    if rung == COMBINED:
        return t + 9e11, 1e-3
    name, _, rest = rung.partition("=")
    if name == "gamma":
        return t, float(rest)
    if name == "offset":
        return t + float(rest), 1.0
    if name == "spread":  # u * S with u[0] = 0 and u[1] = 1: max - min is S exactly
        S, _, gamma = rest.partition(",gamma=")
        lo, hi = float(np.min(t)), float(np.max(t))
        u = (t - lo) / (hi - lo)
        u[0], u[1] = 0.0, 1.0
        return u * float(S), float(gamma)
    if name == "sigma":
        rng = np.random.default_rng([_KIND_ID[kind], n, 99])
        return rng.normal(0.0, float(rest), n), 1.0
    raise KeyError(rung)


def ladder_budgets(rung):
    return (0.5,) if rung == COMBINED else (0.02, 0.5)


def targets_for(n):
    """Group b: below zero, the ends, the middle, high budgets, and past the end (rocco/dp.py:101 clamps)."""
    return [-3, 0, 1, n // 2, int(np.floor(0.9 * n)), int(np.floor(0.999 * n)), n - 1, n, n + 5]


def inside_gates(scores, gamma_or_costs):
    """search.cpp's fast_path_applicable restated: False means the sequential exact kernel MUST answer (path 2)."""
    s = np.asarray(scores, dtype=np.float64)
    if s.size > 1:
        c = np.asarray(gamma_or_costs, dtype=np.float64)
        if not (float(np.min(c)) >= 1e-3 and float(np.max(c)) <= 1e6):
            return False
    lo, hi = float(np.min(s)), float(np.max(s))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return False
    return hi - lo <= 1e9 and max(abs(lo), abs(hi)) <= 1e12


def value_tolerance(oracle_value, count, scores, penalty, sequential=False):
    """tests/tools/fuzz_parity.py's rule: the penalised value is a difference of sums of magnitude
    count * (|s| + |penalty|), and both sides round there.  `sequential`: the value was formed as the CPU harness forms
    it (tests/host_logic/harness.cpp: the objective added up locus by locus, then - penalty * count), whose n additions
    each round a partial sum of up to n * max|s|."""
    with np.errstate(over="ignore", invalid="ignore"):
        top = float(np.max(np.abs(scores)))
        tol = 1e-9 * max(1.0, abs(oracle_value)) + 8.0 * 2.0 ** -52 * max(1, count) * (top + abs(penalty))
        if sequential:
            tol += 2.0 ** -53 * float(len(scores)) ** 2 * top
        return tol


def values_agree(value, oracle_value, count, scores, penalty, exact, sequential=False):
    """`exact`: the sequential exact kernel answered, whose value is the reference's bit for bit (include/rocco_hip.h).
    Two non-finite values agree when they are the same non-finite value."""
    if exact or not (np.isfinite(value) and np.isfinite(oracle_value)):
        return bool(np.array_equal(np.float64(value), np.float64(oracle_value), equal_nan=True))
    return abs(value - oracle_value) <= value_tolerance(oracle_value, count, scores, penalty, sequential)


def fixed_penalties(scores, calibrated):
    """Group e: outside the scores on both sides, inside, absurdly far, exactly on a score, and on / next to the
    penalty a calibration returned."""
    s = np.asarray(scores, dtype=np.float64)
    with np.errstate(over="ignore"):
        out = [float(np.min(s)) - 1.0, float(np.max(s)) + 1.0, float(np.median(s)), 1e300, -1e300, float(s[s.size // 3]),
               float(calibrated), float(np.nextafter(calibrated, -np.inf)), float(np.nextafter(calibrated, np.inf))]
    return [x for x in out if np.isfinite(x)]
