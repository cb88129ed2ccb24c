"""Host side of the post-hoc peak scoring off its defaults (no GPU).  Two things are established here for
tests/test_gpu_peak_scores.py: that the NumPy restatement of tests/peak_scores_expected.py is what the reference's own
helpers computed (tests/golden/scores_offdefault_vectors.npz, written by tests/golden/make_golden_scores.py), and that
the shared inputs can tell a wrong kernel from a right one -- by arithmetic that touches no code of the package."""
import os

import numpy as np
import pytest

import peak_scores_expected as E

HERE = os.path.dirname(os.path.abspath(__file__))
# The reference takes NumPy's log2, the restatement the correctly rounded one.  The largest |difference| between the
# restatement with np.log2 and with the correctly rounded logarithm over the finite results of ALL cases, measured on the
# recording host (NumPy 2.2.6, x86-64), is 3.552713678800501e-15 = 2^-48: one place of a statistic in [16, 32), the
# largest the cases reach (log2(1e6 * count + pc)).  Twice that, because another host's log2 may round the other way.
# (tests/test_gpu_peak_scores.py holds the defaults' fixture to rtol=4e-16, atol=1e-15: statistics below 16.)
LOG2_ATOL = 2 * 3.552713678800501e-15


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "scores_offdefault_vectors.npz")) as data:
        return {key: data[key] for key in data.files}


def matches_recorded(got, recorded) -> bool:
    """NaN where NaN was recorded, the same infinity where one was, within LOG2_ATOL where the record is finite."""
    finite = np.isfinite(recorded)
    return bool(got.shape == recorded.shape and E.same_values(got[~finite], recorded[~finite])
                and np.all(np.abs(got[finite] - recorded[finite]) <= LOG2_ATOL))


def test_the_cases_cover_what_they_are_meant_to():
    cases = E.shape_cases()
    assert {(c["P"], c["K"]) for c in cases} == {(P, K) for P in E.PS for K in E.KS} and len(cases) == 50
    for kind in E.KINDS:
        mine = [c for c in cases if c["kind"] == kind]
        assert {c["K"] for c in mine} == set(E.KS) and {c["P"] for c in mine} == set(E.PS), kind
        assert {pc for c in mine for pc, _ in E.parameters(c)} == set(E.PCS)
        assert {(pc, rs) for c in mine for pc, rs in E.parameters(c)} == {(pc, rs) for pc in E.PCS for rs in E.ROW_SCALES}, kind
    assert any(c["P"] * c["K"] % 256 != 0 and c["P"] * c["K"] > 256 for c in cases)
    for c in cases:
        counts, lengths = E.inputs(c)
        assert counts.shape == (c["P"], c["K"]) and lengths.shape == (c["P"],)
        if c["kind"] in ("integer", "mostly_zero"):
            assert np.array_equal(counts, np.floor(counts)) and counts.min() >= 0
        if c["kind"] == "mostly_zero":
            assert ((counts == 0).mean(axis=1) >= 0.6).all()
        if c["kind"] == "with_inf":
            assert np.isinf(counts).any() and not np.isnan(counts).any()
        if c["kind"] == "with_nan":
            assert np.isnan(counts).any() and np.isnan(counts).sum(axis=1).max() == 1
        if c["P"] >= len(E.LENGTHS):
            assert set(E.LENGTHS) <= set(lengths.tolist())
    fixture = [cases[i] for i in E.FIXTURE_CASES]
    assert all(c["K"] <= 33 and c["P"] <= 257 for c in fixture)
    assert sorted(c["kind"] for c in fixture) == sorted(E.KINDS * 2)
    assert {pc for c in fixture for pc, _ in E.parameters(c)} == set(E.PCS)
    assert {rs for c in fixture for _, rs in E.parameters(c)} == set(E.ROW_SCALES)


def test_the_restatement_is_what_the_reference_recorded(golden):
    cases = E.shape_cases()
    assert tuple(golden["case_indexes"]) == E.FIXTURE_CASES
    assert np.array_equal(golden["percentiles"], np.array(E.PERCENTILES, dtype=np.float64))
    compared = exact = 0
    for index in E.FIXTURE_CASES:
        case = cases[index]
        counts, lengths = E.inputs(case)
        counts, lengths = counts[:E.FIXTURE_ROWS], lengths[:E.FIXTURE_ROWS]
        # the builders still draw what the reference was given
        assert E.same_values(counts, golden[f"case{index}_counts"]) and E.same_values(lengths, golden[f"case{index}_lengths"])
        for j, (pc, row_scale) in enumerate(E.parameters(case)):
            assert np.array_equal(golden[f"case{index}_params{j}"], [pc, row_scale])
            recorded = golden[f"case{index}_sig{j}"]
            assert recorded.shape == (len(E.PERCENTILES), counts.shape[0])
            # the restatement with this host's np.log2 (what the reference calls) and with the correctly rounded one
            assert matches_recorded(E.signal(counts, lengths, row_scale, pc, E.PERCENTILES, log2=np.log2), recorded), (index, j)
            mine = E.expected_signal(case, pc, row_scale)[:, :E.FIXTURE_ROWS]
            assert matches_recorded(mine, recorded), (index, j)
            finite = np.isfinite(recorded)
            compared += int(finite.sum())
            exact += int((mine[finite] == recorded[finite]).sum())
            # one call per percentile, one row at a time, as the reference makes them: the same values as the batched call
            for i, percentile in enumerate(E.PERCENTILES):
                alone = np.array([E.signal(counts[r:r + 1], lengths[r:r + 1], row_scale, pc, percentile)[0]
                                  for r in range(min(counts.shape[0], 5))])
                assert E.same_values(alone, mine[i, :alone.size]), (index, j, percentile)
    assert compared > 5000 and exact > 0.9 * compared  # (NumPy's log2 is the correctly rounded one nearly everywhere)


def test_the_tolerance_is_twice_the_measured_distance_between_the_two_logarithms():
    largest = 0.0
    for case in E.shape_cases():
        counts, lengths = E.inputs(case)
        for pc, row_scale in E.parameters(case):
            want = E.expected_signal(case, pc, row_scale)
            numpys = E.signal(counts, lengths, row_scale, pc, E.PERCENTILES, log2=np.log2)
            finite = np.isfinite(want)
            assert E.same_values(numpys[~finite], want[~finite])
            largest = max(largest, float(np.abs(numpys[finite] - want[finite]).max(initial=0.0)))
    print(f"largest |np.log2 restatement - correctly rounded restatement| = {largest!r}")
    # any host's log2 within one place of the correctly rounded one stays inside the tolerance
    assert 0.0 < largest <= LOG2_ATOL / 2


def test_survival_restatement_is_what_the_reference_recorded(golden):
    from rocco_amd.scores import EmpiricalNull

    names = [name for name, _, _ in E.survival_cases()]
    assert list(golden["survival_names"]) == names
    sizes = set()
    for name, null, stat in E.survival_cases():
        assert E.same_values(null, golden[f"survival_{name}_null"]) and E.same_values(stat, golden[f"survival_{name}_stat"])
        recorded = golden[f"survival_{name}_vector"]
        assert np.array_equal(recorded, golden[f"survival_{name}_scalars"])
        assert np.array_equal(E.survival(stat, np.zeros(stat.size, dtype=int), {0: null}), recorded), name
        assert np.array_equal(EmpiricalNull(null).survival(stat), recorded), name
        # what the statistics are there for
        size = null.size
        sizes.add(size)
        # a NaN sorts after every number (and NaN null values sort last: the search stops at the first of them)
        assert np.isnan(stat[0]) and recorded[0] == (np.isnan(null).sum() + 1.0) / (size + 1.0)
        assert stat[1] == np.inf and stat[2] == -np.inf and recorded[2] == 1.0
        on_a_value = np.isin(stat, null[~np.isnan(null)])
        assert on_a_value.any() and (~on_a_value).any()
    assert sizes >= {1, 2} and max(sizes) > 200
    repeated = [np.unique(null[~np.isnan(null)]).size < (~np.isnan(null)).sum() for _, null, _ in E.survival_cases()]
    assert any(repeated)


def test_the_percentiles_can_tell_the_two_rank_rules_apart():
    """`n q + (1 - q) - 1` against NumPy's `(n - 1) q`: for every percentile at which the two can differ at all there is a
    K among the cases where they do, and a row whose percentile then changes -- judged by an emulation of NumPy's
    interpolation that is first shown to BE np.percentile under NumPy's rule."""
    differing_pairs = {percentile: 0 for percentile in E.PERCENTILES}
    changed_rows = dict(differing_pairs)
    for case in E.shape_cases():
        K = case["K"]
        for pc, row_scale in E.parameters(case):
            ordered = np.sort(E.transformed(*E.inputs(case), row_scale, pc), axis=1)
            clean = ~np.isnan(ordered).any(axis=1)
            for percentile, want in zip(E.PERCENTILES, E.expected_signal(case, pc, row_scale)):
                vi_numpy, vi_general = E.virtual_index_numpy(K, percentile), E.virtual_index_general(K, percentile)
                emulated = E.lerp_rows(ordered, *E.brackets(K, vi_numpy))
                assert E.same_values(emulated[clean], want[clean]) and np.isnan(want[~clean]).all(), (case, percentile)
                if vi_general != vi_numpy:
                    other = E.lerp_rows(ordered, *E.brackets(K, vi_general))
                    differing_pairs[percentile] += 1
                    changed_rows[percentile] += int(np.sum(clean & ~(np.isnan(other) & np.isnan(want)) & (other != want)))
    for percentile in E.PERCENTILES:
        if percentile in E.RANK_RULES_AGREE_AT:
            assert differing_pairs[percentile] == 0, percentile  # (why the defaults' tests never noticed)
        else:
            assert differing_pairs[percentile] > 0 and changed_rows[percentile] > 0, percentile
    print("rows whose percentile the rank rule changes:", changed_rows)
    assert set(E.PERCENTILES) - set(E.RANK_RULES_AGREE_AT) == {0.1, 5, 10, 33.3, 90, 95, 99.9}


def test_zero_pseudocount_on_mostly_zero_rows_gives_nan_and_minus_infinity():
    nan_rows = minus_inf_rows = finite_rows = 0
    for case in E.shape_cases():
        if case["kind"] != "mostly_zero":
            continue
        assert not np.isnan(E.inputs(case)[0]).any()  # no NaN goes in
        (row_scale,) = [rs for pc, rs in E.parameters(case) if pc == 0.0]
        want = E.expected_signal(case, 0.0, row_scale)
        nan_rows += int(np.isnan(want).sum())
        minus_inf_rows += int((want == -np.inf).sum())
        finite_rows += int(np.isfinite(want).sum())
        at_75 = want[E.PERCENTILES.index(75)]
        if case["P"] >= 255 and case["K"] >= 2:
            assert np.isnan(at_75).any()  # (what `score_peak_counts`, fixed at 75, then hands to the survival)
    assert nan_rows > 1000 and minus_inf_rows > 100 and finite_rows > 1000


def test_integer_rows_have_equal_and_unequal_bracketing_order_statistics():
    equal = unequal = 0
    for case in E.shape_cases():
        if case["kind"] != "integer" or case["K"] < 2:
            continue
        pc, row_scale = E.parameters(case)[2]
        ordered = np.sort(E.transformed(*E.inputs(case), row_scale, pc), axis=1)
        assert np.isfinite(ordered).all()
        for percentile in E.PERCENTILES:
            prev, nxt, gamma = E.brackets(case["K"], E.virtual_index_numpy(case["K"], percentile))
            if nxt != prev and gamma != 0.0:
                equal += int((ordered[:, prev] == ordered[:, nxt]).sum())
                unequal += int((ordered[:, prev] != ordered[:, nxt]).sum())
    assert equal > 1000 and unequal > 1000


def test_scipy_refuses_the_invalid_p_values_and_takes_the_valid_ones():
    from scipy import stats

    for m in E.BH_SIZES:
        invalid = E.bh_invalid_vectors(m)
        assert len(invalid) == len(E.BH_INVALID) == 3
        for p, bad in zip(invalid, E.BH_INVALID):
            assert p.shape == (m,) and (np.isnan(p).any() if bad != bad else (p == bad).any())
            with pytest.raises(ValueError) as info:
                stats.false_discovery_control(p, method="bh")
            assert str(info.value) == E.BH_ERROR
        vectors = E.bh_vectors(m)
        assert set(vectors) == {"ties", "all_equal", "all_zero", "all_one", "negative_zero"}
        for name, p in vectors.items():
            q = E.bh(p)
            assert q.shape == (m,) and not np.isnan(q).any(), (m, name)
        assert np.signbit(vectors["negative_zero"]).sum() == 1 and (vectors["negative_zero"] >= 0).all()
        if m >= 1023:
            assert np.unique(vectors["ties"]).size <= 11
    # the issue's own example: -0.0 is a zero, not the largest value
    assert np.array_equal(E.bh([0.2, -0.0, 0.5]), E.bh([0.2, 0.0, 0.5])) and E.bh([0.2, -0.0, 0.5])[1] == 0.0
