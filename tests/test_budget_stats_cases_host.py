"""tests/budget_stats_cases.py and tests/golden/budget_long_lag_vectors.npz without a GPU: the conditions the cases of
tests/test_gpu_budget_stats.py rely on are true -- exact sums are exact, rounding merges where a case says so, NaNs have
the bit patterns meant, the stored long-lag cases truncate where they should with pair sums clear of zero, and the
reference's verdicts on non-finite tracks hold both outcomes for every kind of bad value."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import budget_stats_cases as bc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "budget_long_lag_vectors.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- B1 ----
def test_exact_cases_cannot_round():
    worst = bc.exactness_bound(max(bc.EXACT_LENGTHS + (bc.SPIKE_N,)), 512, max(abs(m) for m in bc.EXACT_MEANS + bc.SPIKE_MEANS))
    assert worst < 2 ** 53 and worst == 16385 * (1024 + 14) ** 2
    for mean in bc.EXACT_MEANS + bc.SPIKE_MEANS:
        assert float(2 * mean).is_integer()
    for n in bc.EXACT_LENGTHS:
        x = bc.exact_track(n)
        assert x.dtype == np.float64 and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 512
        if n >= 2:
            assert x.max() == 512 and x.min() == -512
    assert any(float(m).is_integer() and m != 0 for m in bc.EXACT_MEANS) and any(not float(m).is_integer() for m in bc.EXACT_MEANS)


def test_exact_sums_are_the_rational_sums_and_float_sums_agree_in_any_order():
    x = bc.exact_track(5120)
    for mean in bc.EXACT_MEANS:
        want = bc.exact_sums(x, mean, 40)
        c = x - mean
        for k in (0, 1, 7, 40):
            exact = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(c[:c.size - k], c[k:]))
            assert Fraction(float(want[k])) == exact
            forward = 0.0
            for a, b in zip(c[:c.size - k], c[k:]):
                forward += a * b
            assert forward == want[k] and float(np.dot(c[:c.size - k][::-1], c[k:][::-1])) == want[k]
    assert np.array_equal(bc.exact_sums_all_lags(4097, -2.5)[:41], bc.exact_sums(bc.exact_track(4097), -2.5, 40))


def test_max_lags_cross_every_chunk_and_segment_edge():
    assert bc.max_lags_for(1) == [0] and bc.max_lags_for(2) == [0, 1] and bc.max_lags_for(5) == [0, 1, 2, 4]
    assert bc.max_lags_for(4096) == [0, 1, 2, 255, 256, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 4095]
    full = bc.max_lags_for(16385)
    assert full == sorted(bc.EXACT_MAX_LAGS) + [16384]
    for edge in (bc.CHUNK - 1, bc.CHUNK, bc.CHUNK + 1, 2 * bc.CHUNK, bc.SEG - 1, bc.SEG, bc.SEG + 1):
        assert edge in full
    for edge in (bc.SEG - 1, bc.SEG, bc.SEG + 1, 2 * bc.SEG, 2 * bc.SEG + 1):
        assert edge in bc.EXACT_LENGTHS


def test_spike_tracks_have_one_nonzero_lag():
    cases = bc.spike_cases()
    assert len(cases) == len(set(cases)) >= 29
    assert {p for p, _k in cases} >= {0, 4095, 4096, 8191} and {k for _p, k in cases} == set(bc.SPIKE_LAGS)
    a, b = bc.SPIKE_VALUES
    for p, k in cases:
        assert 0 <= p and p + k < bc.SPIKE_N and k <= bc.SPIKE_MAX_LAG
        assert (bc.SPIKE_N - 1 - k, k) in cases  # the pair that ends at the last locus
        sums = bc.spike_sums(bc.SPIKE_N, p, k, 0.0, bc.SPIKE_MAX_LAG)
        assert sums[k] == a * b and sums[0] == a * a + b * b and np.count_nonzero(sums) == 2
    for p, k in (cases[0], cases[7], cases[-1], (8191, 4097)):  # the closed form is the integer dot product
        for mean in bc.SPIKE_MEANS:
            want = bc.exact_sums(bc.spike_track(bc.SPIKE_N, p, k), mean, bc.SPIKE_MAX_LAG)
            assert np.array_equal(bc.spike_sums(bc.SPIKE_N, p, k, mean, bc.SPIKE_MAX_LAG), want), (p, k, mean)
    # with the half-integer mean every term of every lag is nonzero: a term too few or too many moves the sum
    c = bc.spike_track(bc.SPIKE_N, 0, 1) - bc.SPIKE_MEANS[1]
    assert np.all(c != 0) and bc.SPIKE_MEANS[1] != 0 and not float(bc.SPIKE_MEANS[1]).is_integer()


# ---- B2 ----
def test_real_tracks_and_their_bound():
    for n in bc.REAL_LENGTHS:
        assert n % bc.SEG != 0 and n > 2 * bc.SEG
        lags = bc.real_lags(n)
        assert len(lags) == 10 and lags[-1] == n - 1 and len(set(lags)) == 10
        for kind in ("gamma", "ramp"):
            x = bc.real_track(kind, n)
            assert x.shape == (n,) and np.all(np.isfinite(x)) and not np.array_equal(x, np.round(x))
    m = bc.SEG + 3 + 1
    assert bc.real_bound(8193, Fraction(1)) == Fraction(m, 2 ** 53) / (1 - Fraction(m, 2 ** 53))
    assert bc.real_bound(12289, Fraction(1)) > bc.real_bound(8193, Fraction(1))
    # the reference sums are exact: a short track against integer arithmetic
    x = np.array([0.1, 0.7, -0.3, 0.25, 1.5])
    ref = bc.real_reference(x, 0.2, [0, 2])
    c = [Fraction(float(v)) for v in (x - 0.2)]
    assert ref[2][0] == c[0] * c[2] + c[1] * c[3] + c[2] * c[4] and ref[0][1] == sum(v * v for v in c)
    # and a sequential float sum of the real track stays inside the bound (the bound is not vacuous: it is ~5e-13 relative)
    x = bc.real_track("ramp", 8193)
    mean = float(np.mean(x))
    total, absolute = bc.real_reference(x, mean, [1])[1]
    c, acc = x - mean, 0.0
    for i in range(c.size - 1):
        acc += c[i] * c[i + 1]
    assert abs(Fraction(acc) - total) <= bc.real_bound(8193, absolute) < Fraction(1, 10 ** 12) * absolute


# ---- C ----
def test_long_lag_cases_truncate_where_they_should(gold):
    assert bc.PAIR_MARGIN == 1.0e-6
    seen = set()
    for n in bc.RAMP_LENGTHS:
        assert np.array_equal(gold[f"ramp_n{n}_scores"], bc.ramp_track(n))
        for max_lag in bc.ess_max_lags(n):
            name = f"ramp_n{n}_ess{max_lag}"
            assert name in gold["ess_names"]
            _ess, _tau, used = gold[f"{name}_result"]
            wanted, margin, _last = gold[f"{name}_check"]
            assert wanted == bc.wanted_lags_above(n, max_lag) and used > wanted and used <= max_lag and margin > bc.PAIR_MARGIN
            seen.add((n, int(wanted)))
        for hint in bc.ESTIMATE_HINTS:
            name = f"ramp_n{n}_h{hint}"
            assert name in gold["estimate_names"]
            det = json.loads(str(gold[f"{name}_details"][0]))
            wanted, margin, _last = gold[f"{name}_check"]
            assert det["ess_max_lag"] == min(4 * hint, n - 1)
            assert wanted == bc.wanted_lags_above(n, int(det["ess_max_lag"])) and det["ess_lags_used"] > wanted and margin > bc.PAIR_MARGIN
    assert len(gold["ess_names"]) == 18 and len(gold["estimate_names"]) == 9
    # past one lag chunk, past two, past the segment length -- and the caps at the chunk edge used up
    for n in bc.RAMP_LENGTHS:
        assert {(n, 1022), (n, 1023), (n, 1024), (n, 2048)} <= seen
    assert (8193, 2048) in seen and (12289, 4096) in seen and (16385, 4096) in seen
    for n in bc.RAMP_LENGTHS:  # the free-running truncation lags stop well inside the track
        assert gold[f"ramp_n{n}_ess{n - 1}_result"][2] < n // 2


def test_pair_sums_can_be_recomputed_from_the_stored_track(gold):
    n = 8193
    det = json.loads(str(gold[f"ramp_n{n}_h2000_details"][0]))
    soft = bc.soft_counts(gold[f"ramp_n{n}_scores"], det["null_center"], det["null_scale"])
    pairs, used, tau = bc.geyer_pairs(soft, int(det["ess_max_lag"]))
    assert used == int(det["ess_lags_used"]) and pairs[-1] <= 0.0 and np.all(pairs[:-1] > 0.0)
    assert np.min(np.abs(pairs)) == gold[f"ramp_n{n}_h2000_check"][1] > bc.PAIR_MARGIN
    assert abs(tau - det["autocorrelation_time"]) <= 1e-12 * tau


# ---- D ----
def test_nan_bit_patterns():
    assert np.float64(bc.NEG_NAN).view(np.uint64) == 0xFFF8000000000000 and np.isnan(bc.NEG_NAN)
    assert np.float64(np.nan).view(np.uint64) == 0x7FF8000000000000
    assert np.float64(bc.BAD_VALUES["negnan"]).view(np.uint64) >> np.uint64(63) == 1
    assert np.float64(bc.BAD_VALUES["nan"]).view(np.uint64) >> np.uint64(63) == 0
    values = bc.SPECIAL_BITS.view(np.float64)
    nan_bits = bc.SPECIAL_BITS[np.isnan(values)]
    assert nan_bits.size == 8 and (nan_bits >> np.uint64(63)).sum() == 4 and np.unique(nan_bits).size == 8
    assert np.unique(bc.SPECIAL_BITS).size == bc.SPECIAL_BITS.size


def test_sort_key_orders_values_and_brackets_them_with_nans():
    ordered = bc.expected_sorted_bits(bc.SPECIAL_BITS)
    v = ordered.view(np.float64)
    nan = np.isnan(v)
    assert nan[:4].all() and nan[-4:].all() and not nan[4:-4].any()
    assert (ordered[:4] >> np.uint64(63) == 1).all() and (ordered[-4:] >> np.uint64(63) == 0).all()
    body = v[4:-4]
    assert body[0] == -np.inf and body[-1] == np.inf and np.all(np.diff(body) >= 0)
    zeros = np.flatnonzero(body == 0)
    assert np.signbit(body[zeros[0]]) and not np.signbit(body[zeros[1]])
    rng = np.random.default_rng(3)
    finite = rng.normal(size=1000)
    assert np.array_equal(bc.expected_sorted_bits(finite.view(np.uint64)).view(np.float64), np.sort(finite))


@pytest.mark.parametrize("n", bc.SORT_LENGTHS)
def test_sort_inputs_are_what_their_kinds_say(n):
    for kind in bc.SORT_KINDS:
        bits = bc.sort_input_bits(kind, n)
        assert bits.dtype == np.uint64 and bits.shape == (n,)
        assert np.array_equal(np.sort(bc.expected_sorted_bits(bits)), np.sort(bits))  # a permutation
    assert np.unique(bc.sort_input_bits("one-value", n)).size == 1
    assert np.unique(bc.sort_input_bits("sixteen-values", n)).size <= 16
    if n >= 255:
        assert np.unique(bc.sort_input_bits("sixteen-values", n)).size == 16
        assert np.isin(bc.SPECIAL_BITS, bc.sort_input_bits("specials", n)).all()
        v = bc.sort_input_bits("bits", n).view(np.float64)
        assert (np.signbit(v)).any() and (~np.signbit(v)).any()
    if n >= 4096:
        v = bc.sort_input_bits("bits", n).view(np.float64)
        assert np.isnan(v).any() and (np.abs(v[np.isfinite(v)]) < 2.3e-308).any()  # NaNs and denormals among random bits


def test_probe_vectors_and_the_rounding_merge():
    vectors = bc.probe_vectors()
    for name, x in vectors.items():
        assert not np.isnan(x).any() and np.array_equal(bc.expected_sorted_bits(x.view(np.uint64)).view(np.float64), x, equal_nan=True), name
    ties = vectors["ties"]
    assert [int((ties == v).sum()) for v in (0.5, 1.75, -1.125)] == [1, 2, 1000]
    zeros = ties[ties == 0]
    assert zeros.size == 4 and np.signbit(zeros[:2]).all() and not np.signbit(zeros[2:]).any()
    assert ties[0] == -np.inf and ties[-1] == ties[-2] == np.inf
    assert vectors["one"].size == 1 and vectors["two"].size == 2 and vectors["big"].size > 2 ** 16
    x, shift = bc.merging_case()
    assert np.unique(x).size == x.size == 64 and np.unique(x - shift).size <= 17  # neighbours merge
    assert (np.diff(x - shift) >= 0).all()
    x, shift = bc.cancelling_case()
    assert np.unique(x - shift).size == x.size  # exact: none merge
    # thresholds: each kind is present
    thresholds = bc.probe_thresholds(ties)
    le, lt = bc.probe_counts(ties, 0.0, thresholds)
    equal = [a - b for a, b in zip(le, lt)]
    assert {1000, 2, 1, 0} <= set(equal) and equal[thresholds.index(1.75)] == 2 and equal[thresholds.index(-1.125)] == 1000
    assert 0 in lt and ties.size in le and np.inf in thresholds and -np.inf in thresholds
    big_le, big_lt = bc.probe_counts(vectors["big"], 0.0, bc.probe_thresholds(vectors["big"]))
    assert 0 in big_le and vectors["big"].size in big_lt  # below the minimum, above the maximum
    at_zero = thresholds.index(0.0)
    assert le[at_zero] - lt[at_zero] == 4  # both zeros count as equal to 0.0


def test_elementwise_inputs():
    for n in bc.ELEMENTWISE_LENGTHS:
        v = bc.elementwise_input(n)
        assert v.shape == (n,) and np.isfinite(v).all()
        if n >= 255:
            assert (v == bc.CENTER).any() and np.signbit(v[v == 0]).any() and (np.abs(v[v != 0]) < 1e-320).any()
    assert bc.elementwise_input(1)[0] == bc.CENTER
    assert len(repr(bc.CENTER)) >= 17 and len(repr(bc.SCALE)) >= 17


# ---- E ----
def test_census_of_the_reference_verdicts(gold):
    verdicts = json.loads(str(gold["nonfinite_verdicts"][0]))
    tracks = dict(bc.nonfinite_tracks())
    assert set(verdicts) == set(tracks) and len(tracks) == 26
    for name, s in tracks.items():
        bad = bc.BAD_VALUES[bc.bad_class(name)]
        hit = np.isnan(s) if np.isnan(bad) else (s == bad)
        want = {"tenth": s.size // 10, "all": s.size}.get(name.split("_")[-1], 1)
        assert int(hit.sum()) == want and np.isfinite(s[~hit]).all(), name
        if bc.bad_class(name) == "negnan":
            assert (s[hit].view(np.uint64) >> np.uint64(63) == 1).all()
    outcomes = {bad: set() for bad in bc.BAD_VALUES}
    for name, by_function in verdicts.items():
        for function, v in by_function.items():
            assert set(v) in ({"raises", "message"}, {"returns"})
            outcomes[bc.bad_class(name)].add((function, "raises" if "raises" in v else "returns"))
    for bad, seen in outcomes.items():  # each of "raises" and "returns" at least once per kind of bad value
        assert {o for _f, o in seen} == {"raises", "returns"}, (bad, seen)
    refused = "Direct-score budget null fit produced non-finite values"
    for name, by_function in verdicts.items():
        e, bad = by_function["estimate"], bc.bad_class(name)
        if bad != "neginf":  # NaN of either sign and +inf: refused, always with this message
            assert e.get("raises") == "ValueError" and e["message"] == refused, name
        assert "returns" in by_function["ess"] and by_function["ess"]["returns"][1:] == [1.0, 0.0]
        assert "returns" in by_function["gamma"]
    # one -inf: an answer on the long track and at the head of the short one, refused where the scale comes out infinite
    for where in ("first", "middle", "last"):
        assert "returns" in verdicts[f"neginf_signal_{where}"]["estimate"]
        assert np.isnan(verdicts[f"neginf_signal_{where}"]["estimate"]["returns"]["details"]["null_excess_units"])
    assert "returns" in verdicts["neginf_short_first"]["estimate"]
    assert verdicts["neginf_short_middle"]["estimate"]["message"] == verdicts["neginf_short_last"]["estimate"]["message"] == refused
    # the switch cost ignores NaNs and keeps +inf among the positive scores
    clean = float(np.sum(bc.signal_track() > 0))
    assert verdicts["nan_signal_first"]["gamma"]["returns"][4] == verdicts["negnan_signal_last"]["gamma"]["returns"][4] == clean - 1
    assert verdicts["posinf_signal_middle"]["gamma"]["returns"][4] == clean
    assert verdicts["nan_signal_tenth"]["gamma"]["returns"][4] == clean - 400 and verdicts["nan_signal_all"]["gamma"]["returns"][3:5] == [1.0, 0.0]
    assert verdicts["posinf_short_last"]["gamma"]["returns"][3] == np.inf
