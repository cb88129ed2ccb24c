"""CPU: the oracle's restatement of the cross-fit Whittaker baseline (oracle/baseline_oracle.c) against
the golden vectors written from the reference's own backend, and against the recorded outputs of that backend on
seeded inputs (tests/reference_record.py); plus the host helpers of rocco_amd.inference."""
import os

import numpy as np

import reference_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "baseline_vectors.npz")


def oracle_baseline(oracle, matrix, lam):
    return oracle.crossfit_whittaker_baseline(matrix, lam)


def test_oracle_reproduces_golden_baselines_bit_for_bit(oracle):
    gold = np.load(GOLD)
    for name in gold["names"]:
        got = oracle_baseline(oracle, gold[f"{name}_matrix"], float(gold[f"{name}_lambda"]))
        assert got.tobytes() == gold[f"{name}_baseline"].tobytes(), name


def reference_backend_cases():
    """(case name, matrix, lambda): the seeded inputs on which the reference's backend was recorded."""
    rng = np.random.default_rng(5)
    for n in (1, 3, 24, 25, 27, 100, 4097, 33333):
        for lam in (0.36, 4.67e5, 1e-3, 1e9):
            yield f"n={n} lambda={lam!r}", np.ascontiguousarray(rng.normal(0, 1, (2, n)) * rng.choice([1, 100])), lam


def test_oracle_matches_compiled_reference_backend(oracle):
    """The reference's rocco_crossfit_whittaker_baseline_matrix_f64, bit for bit."""
    want = reference_record.recorded("baseline_backend")
    for name, m, lam in reference_backend_cases():
        assert reference_record.digest(oracle_baseline(oracle, m, lam)) == want[name], name


def test_window_and_penalty_rules():
    from rocco_amd.inference import _consenrich_whittaker_lambda, _resolve_local_baseline_window

    # rocco/inference.py:49-76
    assert _resolve_local_baseline_window(24) == 0
    assert _resolve_local_baseline_window(25) == 25
    assert _resolve_local_baseline_window(26, 101) == 25
    assert _resolve_local_baseline_window(1000, 101) == 101
    assert _resolve_local_baseline_window(1000, 100) == 101
    assert _consenrich_whittaker_lambda(101) == 7.0 * ((101.0 * 0.15915494) ** 4)
    assert _consenrich_whittaker_lambda(100) == _consenrich_whittaker_lambda(101)
    assert _consenrich_whittaker_lambda(1) == _consenrich_whittaker_lambda(3)
