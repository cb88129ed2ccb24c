"""GPU: the kernels of rocco_amd/csrc/budget_stats.hip called directly -- autocovariance sums against exact integer sums
at every lag chunk (1024 lags) and segment (4096 loci) edge and against exact rational sums under a derived bound; the
radix sort of doubles against the order of the bit patterns, every payload intact; the sorted probe on ties, merges and
the limits of its arguments; negative part and soft counts against NumPy -- and rocco_amd.budget past 1023 lags and on
non-finite tracks against the reference's own outputs and verdicts (tests/golden/make_golden_budget_long_lag.py).
Cases and expected values: tests/budget_stats_cases.py, checked without a GPU by tests/test_budget_stats_cases_host.py."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import budget_stats_cases as bc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "budget_long_lag_vectors.npz")
FROM_AUTOCORRELATION = {"autocorrelation_time", "effective_total_count", "effective_count"}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _device(x, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _autocov(x_t, mean, max_lag, solver=None, n=None):
    """(return code, sums[0..max_lag]) of rocco_hip_autocovariance_sums_f64, called as budget.py calls it."""
    from rocco_amd import _native, dp

    lib = _native.load()
    solver = solver or _native.solver_for(x_t.device.index)
    sums = (ctypes.c_double * (max(max_lag, 0) + 1))()
    rc = lib.rocco_hip_autocovariance_sums_f64(solver.handle, x_t.data_ptr(), int(x_t.shape[0]) if n is None else n, float(mean),
                                               int(max_lag), sums, dp._stream_ptr(x_t))
    return rc, np.array(sums[:], dtype=np.float64)


def _first_difference(got, want):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    return None if bad.size == 0 else (int(bad[0]), float(got[bad[0]]), float(want[bad[0]]), int(bad.size))


# ---- B1 ----
@pytest.mark.parametrize("n", bc.EXACT_LENGTHS)
def test_autocovariance_sums_exact_at_every_lag(gpu, n):
    x_t = _device(bc.exact_track(n), gpu)
    for mean in bc.EXACT_MEANS:
        want = bc.exact_sums_all_lags(n, mean)
        for max_lag in bc.max_lags_for(n):
            rc, got = _autocov(x_t, mean, max_lag)
            assert rc == 0, (n, mean, max_lag, rc)
            assert _first_difference(got, want[:max_lag + 1] + 0.0) is None, (n, mean, max_lag, _first_difference(got, want[:max_lag + 1] + 0.0))


@pytest.mark.parametrize("mean", bc.SPIKE_MEANS)
def test_autocovariance_sums_of_two_spikes(gpu, mean):
    n = bc.SPIKE_N
    for p, k in bc.spike_cases():
        want = bc.spike_sums(n, p, k, mean, bc.SPIKE_MAX_LAG)
        rc, got = _autocov(_device(bc.spike_track(n, p, k), gpu), mean, bc.SPIKE_MAX_LAG)
        assert rc == 0
        if mean == 0.0:
            a, b = bc.SPIKE_VALUES
            assert got[k] == a * b and got[0] == a * a + b * b and np.count_nonzero(got) == 2, (p, k, np.flatnonzero(got))
        assert _first_difference(got, want + 0.0) is None, (p, k, mean, _first_difference(got, want + 0.0))


# ---- B2 ----
@pytest.mark.parametrize("n", bc.REAL_LENGTHS)
@pytest.mark.parametrize("kind", ["gamma", "ramp"])
def test_autocovariance_sums_within_the_derived_bound(gpu, kind, n):
    x = bc.real_track(kind, n)
    mean = float(np.mean(x))
    lags = bc.real_lags(n)
    reference = bc.real_reference(x, mean, lags)
    rc, got = _autocov(_device(x, gpu), mean, n - 1)
    assert rc == 0
    for k in lags:
        exact, absolute = reference[k]
        error, bound = abs(Fraction(float(got[k])) - exact), bc.real_bound(n, absolute)
        print(f"{kind} n={n} lag {k}: |got - exact| = {float(error):.3e}, bound {float(bound):.3e}, relative to |sum| {float(error / abs(exact)):.2e}")
        assert error <= bound, (kind, n, k, float(error), float(bound))


# ---- B3 ----
def test_autocovariance_scratch_reuse(gpu):
    from rocco_amd import _native

    solver = _native.Solver(gpu.index)
    try:
        for n, max_lag, seed in ((12289, 5119, None), (4097, 3, 99), (12289, 5119, None)):
            x = bc.exact_track(n, seed)
            rc, got = _autocov(_device(x, gpu), -2.5, max_lag, solver=solver)
            assert rc == 0
            want = bc.exact_sums(x, -2.5, max_lag)
            assert _first_difference(got, want + 0.0) is None, (n, max_lag, _first_difference(got, want + 0.0))
    finally:
        solver.close()


# ---- B4 ----
def test_autocovariance_argument_checks(gpu):
    from rocco_amd import _native, dp

    x_t = _device(bc.exact_track(5), gpu)
    assert _autocov(x_t, 0.0, -1)[0] == _native.EINVAL
    assert _autocov(x_t, 0.0, 5)[0] == _native.EINVAL and _autocov(x_t, 0.0, 6)[0] == _native.EINVAL
    assert _autocov(x_t, 0.0, 0, n=0)[0] == _native.EINVAL
    lib, solver = _native.load(), _native.solver_for(gpu.index)
    assert lib.rocco_hip_autocovariance_sums_f64(solver.handle, x_t.data_ptr(), 5, 0.0, 2, None, dp._stream_ptr(x_t)) == _native.EINVAL
    rc, got = _autocov(x_t, 0.0, 4)  # and the call still works afterwards
    assert rc == 0 and np.array_equal(got, bc.exact_sums(bc.exact_track(5), 0.0, 4))


# ---- C ----
def _same_details(got, want, label):
    assert set(got) == set(want), label
    for key, value in want.items():
        if isinstance(value, (str, bool)):
            assert got[key] == value, (label, key)
        elif key in FROM_AUTOCORRELATION:
            assert np.isclose(got[key], value, rtol=1e-9, atol=1e-12), (label, key, got[key], value)
        else:
            assert got[key] == value or (np.isnan(got[key]) and np.isnan(value)), (label, key, got[key], value)


def _gamma_row(gamma, meta):
    return [gamma, meta["autocorrelation_time"], meta["characteristic_run_length"], meta["positive_score_median"],
            meta["positive_score_count"], meta["gamma_raw"]]


@pytest.mark.parametrize("n", bc.RAMP_LENGTHS)
def test_effective_sample_size_past_1023_lags(gpu, gold, n):
    from rocco_amd.budget import _estimate_effective_sample_size

    det = json.loads(str(gold[f"ramp_n{n}_h256_details"][0]))
    soft = bc.soft_counts(gold[f"ramp_n{n}_scores"], det["null_center"], det["null_scale"])
    for max_lag in bc.ess_max_lags(n):
        ess, tau, lags = _estimate_effective_sample_size(soft, max_lag)
        w_ess, w_tau, w_lags = gold[f"ramp_n{n}_ess{max_lag}_result"]
        print(f"n={n} max_lag={max_lag}: lags {lags} (reference {int(w_lags)}), tau / reference - 1 = {tau / w_tau - 1:.2e}")
        assert lags == int(w_lags), (n, max_lag, lags, w_lags)
        assert np.isclose(tau, w_tau, rtol=1e-9) and np.isclose(ess, w_ess, rtol=1e-9), (n, max_lag, tau, w_tau)


@pytest.mark.parametrize("n", bc.RAMP_LENGTHS)
def test_score_track_estimate_with_long_lag_hints(gpu, gold, n):
    from rocco_amd.budget import _resolve_chrom_gamma, estimate_budget_nonnull_fraction_from_score_track

    scores = gold[f"ramp_n{n}_scores"]
    for hint in bc.ESTIMATE_HINTS:
        name = f"ramp_n{n}_h{hint}"
        fraction, details = estimate_budget_nonnull_fraction_from_score_track(scores, dependence_lag_hint=hint, num_null_draws=6,
                                                                              return_details=True)
        want = json.loads(str(gold[f"{name}_details"][0]))
        assert details["ess_lags_used"] == want["ess_lags_used"] and details["ess_max_lag"] == want["ess_max_lag"], name
        _same_details(details, want, name)
        assert fraction == float(gold[f"{name}_fraction"][0]), name
        gamma, meta = _resolve_chrom_gamma("chrT", {"gamma": None}, scores, details)
        g_want = gold[f"{name}_gamma"]
        assert meta["characteristic_run_length"] == int(g_want[2]) and meta["positive_score_count"] == int(g_want[4]), name
        assert meta["positive_score_median"] == g_want[3] and gamma == g_want[0] and meta["gamma_raw"] == g_want[5], name
        assert np.isclose(meta["autocorrelation_time"], g_want[1], rtol=1e-9), name


# ---- D1 ----
@pytest.mark.parametrize("n", bc.SORT_LENGTHS)
def test_sort_orders_bit_patterns_and_keeps_every_payload(gpu, n):
    import torch
    from rocco_amd.budget import sort_device

    for kind in bc.SORT_KINDS:
        bits = bc.sort_input_bits(kind, n)
        x_t = _device(bits.view(np.int64), gpu).view(torch.float64)
        got = sort_device(x_t).view(torch.int64).cpu().numpy().view(np.uint64)
        want = bc.expected_sorted_bits(bits)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (kind, n, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
        assert np.array_equal(x_t.view(torch.int64).cpu().numpy().view(np.uint64), bits)  # the input is left alone


def test_sort_of_nothing_touches_nothing(gpu):
    import torch
    from rocco_amd import _native, dp
    from rocco_amd.budget import sort_device

    out = torch.full((4,), 7.5, dtype=torch.float64, device=gpu)
    lib, solver = _native.load(), _native.solver_for(gpu.index)
    assert lib.rocco_hip_sort_f64(solver.handle, out.data_ptr(), 0, out.data_ptr(), dp._stream_ptr(out)) == _native.OK
    assert lib.rocco_hip_sort_f64(solver.handle, None, 0, None, dp._stream_ptr(out)) == _native.OK
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.5] * 4
    assert sort_device(torch.empty(0, dtype=torch.float64, device=gpu)).shape == (0,)


# ---- D2 ----
def _chunks(items, size=8):
    return [items[i:i + size] for i in range(0, len(items), size)]


def test_sorted_probe_counts(gpu):
    from rocco_amd.budget import sorted_probe

    vectors = bc.probe_vectors()
    shifts = {name: [0.0, float(x[np.isfinite(x)][x[np.isfinite(x)].size // 2])] for name, x in vectors.items()}
    shifts["merge"].append(bc.merging_case()[1])
    shifts["cancel"].append(bc.cancelling_case()[1])
    shifts["ties"].append(-1.125)
    for name, x in vectors.items():
        x_t = _device(x, gpu)
        for shift in shifts[name]:
            thresholds = bc.probe_thresholds(x - np.float64(shift))
            want_le, want_lt = bc.probe_counts(x, shift, thresholds)
            got_le, got_lt = [], []
            for part in _chunks(thresholds):
                values, le, lt = sorted_probe(x_t, thresholds=part, shift=shift)
                assert values == [] and len(le) == len(lt) == len(part)
                got_le += le
                got_lt += lt
            assert got_le == want_le and got_lt == want_lt, (name, shift, thresholds, got_le, want_le, got_lt, want_lt)


def test_sorted_probe_ranks_and_limits(gpu):
    from rocco_amd.budget import _median_of_sorted_range, sorted_probe

    for name, x in bc.probe_vectors().items():
        x_t, n = _device(x, gpu), x.size
        assert sorted_probe(x_t) == ([], [], [])
        for count in range(1, 9):
            ranks = [-1, n, 0, n - 1, n // 2, n // 3, 1 % n, -5][:count]
            values, le, lt = sorted_probe(x_t, ranks=ranks)
            want = [float(x[r]) if 0 <= r < n else 0.0 for r in ranks]
            assert le == [] and lt == [] and np.array(values).tobytes() == np.array(want).tobytes(), (name, ranks, values, want)
        values, le, lt = sorted_probe(x_t, ranks=list(range(-1, 7)), thresholds=[float(x[0])] * 8)  # 8 of each at once
        assert len(values) == len(le) == len(lt) == 8 and le == [int((x <= x[0]).sum())] * 8 and lt == [0] * 8
        with pytest.raises(ValueError, match="rocco_hip_sorted_probe_f64: invalid argument"):
            sorted_probe(x_t, ranks=[0] * 9)
        with pytest.raises(ValueError, match="rocco_hip_sorted_probe_f64: invalid argument"):
            sorted_probe(x_t, thresholds=[0.0] * 9)
        for first, count in ((0, n), (0, max(1, n - 1)), (n // 3, n - n // 3), (n // 3, max(1, n - n // 3 - 1)), (n - 1, 1)):
            with np.errstate(invalid="ignore"):
                want = float(np.median(x[first:first + count]))
            got = _median_of_sorted_range(x_t, first, count)
            assert got == want or (np.isnan(got) and np.isnan(want)), (name, first, count, got, want)


def test_sorted_probe_keeps_nans_at_the_ends(gpu):
    """The sort puts sign-set NaNs first and the others last; the probe's search must not be led astray by them (a NaN
    satisfies no comparison): counts are indices into the sorted vector, the leading NaNs included."""
    from rocco_amd.budget import sort_device, sorted_probe

    rng = np.random.default_rng(8)
    for lead, trail in ((3, 0), (0, 5), (700, 1300), (1, 1)):
        body = np.concatenate([np.round(rng.normal(size=1000), 2), [-np.inf, np.inf, 0.0, -0.0]])
        x = np.concatenate([np.full(trail, np.nan), body, np.full(lead, bc.NEG_NAN)])
        ordered = sort_device(_device(x, gpu))
        thresholds = [0.0, -np.inf, np.inf, 0.25, -3.0, 1.0e9]
        _, le, lt = sorted_probe(ordered, thresholds=thresholds)
        assert le == [lead + int((body <= t).sum()) for t in thresholds], (lead, trail, le)
        assert lt == [lead + int((body < t).sum()) for t in thresholds], (lead, trail, lt)
        assert lt[1] == lead and le[2] == lead + body.size


# ---- D3 ----
@pytest.mark.parametrize("n", bc.ELEMENTWISE_LENGTHS)
def test_negative_part_and_soft_counts(gpu, n):
    import torch
    from rocco_amd import _native, dp

    v = bc.elementwise_input(n)
    v_t, out = _device(v, gpu), torch.full((n + 1,), 123.0, dtype=torch.float64, device=gpu)
    lib, solver, stream = _native.load(), _native.solver_for(gpu.index), dp._stream_ptr(out)

    def same(got, want, what):
        assert np.array_equal(got, want), (what, n, np.flatnonzero(got != want)[:5])
        nonzero = want != 0
        assert np.array_equal(np.signbit(got[nonzero]), np.signbit(want[nonzero])), (what, n)

    assert lib.rocco_hip_negative_part_f64(solver.handle, v_t.data_ptr(), out.data_ptr(), n, stream) == _native.OK
    got = out.cpu().numpy()
    assert got[n] == 123.0
    same(got[:n], bc.negative_part(v), "negative_part")
    for center, scale in ((bc.CENTER, bc.SCALE), (0.0, 1.0e-6), (-bc.CENTER, 1.0 / 3.0)):
        assert lib.rocco_hip_soft_counts_f64(solver.handle, v_t.data_ptr(), center, scale, out.data_ptr(), n, stream) == _native.OK
        got = out.cpu().numpy()
        assert got[n] == 123.0
        with np.errstate(over="ignore"):
            same(got[:n], bc.soft(v, center, scale), f"soft_counts({center}, {scale})")
    for scale in (0.0, -1.0, float("nan"), -0.0):
        assert lib.rocco_hip_soft_counts_f64(solver.handle, v_t.data_ptr(), 0.0, scale, out.data_ptr(), n, stream) == _native.EINVAL


# ---- E ----
@pytest.fixture(scope="module")
def verdicts(gold):
    return json.loads(str(gold["nonfinite_verdicts"][0]))


def _verdict(call):
    try:
        return {"returns": call()}
    except Exception as exc:  # noqa: BLE001 (the verdict IS the exception)
        return {"raises": type(exc).__name__, "message": str(exc)}


@pytest.mark.parametrize("bad", list(bc.BAD_VALUES))
def test_non_finite_tracks_get_the_reference_verdict(gpu, verdicts, bad):
    from rocco_amd.budget import (_estimate_effective_sample_size, _resolve_chrom_gamma,
                                  estimate_budget_nonnull_fraction_from_score_track)

    for name, s in bc.nonfinite_tracks():
        if bc.bad_class(name) != bad:
            continue
        want = verdicts[name]
        got = _verdict(lambda: estimate_budget_nonnull_fraction_from_score_track(s, num_null_draws=6, return_details=True))
        if "raises" in want["estimate"]:
            assert got.get("raises") == want["estimate"]["raises"] and got["message"] == want["estimate"]["message"], (name, got)
        else:
            assert "returns" in got, (name, got)
            fraction, details = got["returns"]
            _same_details(details, want["estimate"]["returns"]["details"], name)
            assert fraction == want["estimate"]["returns"]["fraction"], name
        got = _verdict(lambda: [float(v) for v in _estimate_effective_sample_size(s, bc.NONFINITE_ESS_MAX_LAG)])
        assert got == want["ess"], (name, got, want["ess"])
        got = _verdict(lambda: _gamma_row(*_resolve_chrom_gamma("chrT", {"gamma": None}, s, {"autocorrelation_time": 3.25})))
        assert "returns" in got and [float(v) for v in got["returns"]] == want["gamma"]["returns"], (name, got, want["gamma"])
