"""Inputs shared by the tests that take the calibration off the reference's default of 60 bisection steps
(tests/test_gpu_calibration_steps.py on the GPU, the off-sixty tests of tests/test_host_logic.py on the CPU): the step
counts, the batches, and the regimes a step count puts a bisection in, told from the oracle's answers alone.

`max_iter` (rocco/dp.py:93,141) reaches search.cpp (tree depths, the last tree, the zone / spine endgame), budget.hip
(the number of rounds of a rounding-model chain, clamped at 16) and the director of the rounding-model chain
(model_chain.hip: the device's own two replays of the bisection, plan_round and the walk that follows a round; the
threshold chain of chain.hip does not know it), so every step count here is meant to land in a different part of them.
Tracks and the rule for the penalised value are those of tests/envelope_cases.py."""
import numpy as np

import envelope_cases as ec

STEP_COUNTS = (0, 1, 2, 7, 17, 26, 33, 45, 53, 59, 61, 64, 65, 75, 120, 200)
DEVICE_SIDE_STEP_COUNTS = (2, 26, 61, 120)  # the subset run under every imitated device-side behaviour

_ORACLE = {}  # the oracle's answers, computed once and shared by the tests of a session (never modified)


def reference(oracle, key, scores, gamma_or_costs, target, max_iter):
    """oracle.calibrate_selection_penalty(..., max_iter=, return_evaluations=True) of the problem named `key`."""
    key = (key, int(target), int(max_iter))
    if key not in _ORACLE:
        costs = oracle.build_switch_costs(scores, gamma_or_costs) if np.isscalar(gamma_or_costs) else gamma_or_costs
        ref = oracle.calibrate_selection_penalty(scores, costs, target, max_iter=max_iter, return_evaluations=True)
        ref[1].flags.writeable = False
        _ORACLE[key] = ref
    return _ORACLE[key]


# ---- regimes: every predicate takes oracle results (penalty, solution, value, count[, evaluations]) ------------------

def far(ref, target):
    """The bracket is still so wide that its upper end is above every score: nothing is selected."""
    return target > 0 and ref[3] == 0


def cut_open(ref, ref_at_60):
    """The bisection was cut (or carried on) where the count still moves: not the count of 60 steps."""
    return ref[3] != ref_at_60[3]


def past_sixty(ref, ref_at_60):
    """The penalty is not the one 60 steps give."""
    return ref[0] != ref_at_60[0]


def converged(ref, ref_at_next_step_count):
    """More steps no longer move the upper end: the penalty is that of the next larger step count."""
    return ref[0] == ref_at_next_step_count[0]


def regimes(refs, target):
    """`refs`: {max_iter: oracle result} holding 60 and every step count asked about.  -> {max_iter: set of names};
    `converged` compares with the next larger key of `refs`."""
    steps = sorted(refs)
    out = {}
    for k, m in enumerate(steps):
        names = set()
        if far(refs[m], target):
            names.add("far")
        if cut_open(refs[m], refs[60]):
            names.add("cut_open")
        if past_sixty(refs[m], refs[60]):
            names.add("past_sixty")
        if k + 1 < len(steps) and converged(refs[m], refs[steps[k + 1]]):
            names.add("converged")
        out[m] = names
    return out


# (kind, n, target, gamma): the tracks whose oracle answers span every regime (asserted by
# tests/test_host_logic.py::test_step_counts_span_every_regime)
REGIME_TRACKS = (("normal", 262145, 5242, 1.0), ("peaks", 70000, 1400, 1.0), ("integers", 8193, 819, 1.0))

# ---- the batches of the GPU tests -----------------------------------------------------------------------------------

KINDS = ("peaks", "integers", "normal")
# tests/test_gpu_chain.py's batch (without its 8192): short and long, two tiles and one, n = 2 and 3
BATCH_SIZES = (8191, 8193, 70000, 3, 2, 262145)
BATCH_GAMMAS = (1.0, 2.0, 1.0, 1.0, 1.0, 3.0)
BATCH_BUDGETS = (0.02, 0.005, 0.03, 0.5, 0.0, 0.02)
# every problem ends on a compacted level: the rounding-model rounds run as a chain (tests/test_gpu_chain.py)
COMPACTED_SIZES = (300_000, 120_000, 90_000, 500_000)
COMPACTED_BUDGET = 0.02
COMPACTED_KINDS = ("peaks", "normal")
COMPACTED_STEP_COUNTS = (26, 33, 45, 59, 61, 75, 120, 200)


def batch(kind):
    """[(scores, gamma, target)] of the mixed-size batch."""
    return [(ec.track(kind, n), g, int(np.floor(n * b))) for n, g, b in zip(BATCH_SIZES, BATCH_GAMMAS, BATCH_BUDGETS)]


def compacted_batch(kind):
    return [(ec.track(kind, n), 1.0, int(np.floor(n * COMPACTED_BUDGET))) for n in COMPACTED_SIZES]


def host_logic_problem(kind, n, seed):
    """(scores, gamma, target) of the CPU harness's kinds (tests/test_host_logic.py: round5, int, normal, offset)."""
    rng = np.random.default_rng([seed, n, ("round5", "int", "normal", "offset").index(kind)])
    if kind == "round5":
        s = np.round(rng.gamma(1.0, 0.3, n), 5)
        s[rng.integers(0, n, max(1, n // 50))] += rng.gamma(6.0, 1.0, max(1, n // 50))
    elif kind == "int":
        s = rng.integers(-3, 6, n).astype(float)
    elif kind == "normal":
        s = rng.normal(0.2, 1.0, n)
    else:
        s = 1.0e3 + rng.gamma(1.0, 1.0, n)
    gamma = float(rng.choice([0.5, 1.0, 3.0]))
    target = int(np.floor(n * float(rng.choice([0.01, 0.05, 0.2]))))
    return s, gamma, target
