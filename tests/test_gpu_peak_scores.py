"""GPU: the per-peak arithmetic of the post-hoc scoring (rocco_amd/scores.py over peakscore.hip) against outputs of the
reference's own helpers (tests/golden/make_golden_scores.py): `_peak_signal_stat`, `EmpiricalNull.survival` and SciPy's
Benjamini-Hochberg as `score_peaks` applies it.  The signal statistic carries a log2: exact against a restatement with
the correctly rounded logarithm, and against the reference's (NumPy's log2) to the last place.

Off the defaults (percentile, pc, row scale, ties, zeros, infinities, NaNs) the kernels are held to the NumPy / SciPy
restatement of tests/peak_scores_expected.py, which tests/test_peak_scores_host.py pins to the reference's recorded
outputs: equal bits, NaN for NaN, the same infinity, no tolerance."""
import os
import warnings

import numpy as np
import pytest

import peak_scores_expected as E
from log2_truth import log2_correctly_rounded

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scores_vectors.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_scoring_against_the_reference_helpers(gpu, gold):
    from scipy import stats

    from rocco_amd.scores import EmpiricalNull, score_peak_counts

    for name in gold["names"]:
        counts, lengths, binned = gold[f"{name}_counts"], gold[f"{name}_lengths"], gold[f"{name}_binned"]
        nulls = {int(k): EmpiricalNull(gold[f"{name}_null_{int(k)}"]) for k in gold[f"{name}_null_keys"]}
        got = score_peak_counts(counts, lengths, binned, nulls)
        # the statistic with the correctly rounded logarithm, NumPy for the percentile: bit for bit
        factor = 1000.0 / np.maximum(lengths.astype(np.int64), 1).astype(np.float64)
        logged = log2_correctly_rounded(np.maximum(counts * factor[:, None] + 1.0, 1.0))
        assert np.array_equal(got["signal"], np.percentile(logged, 75.0, axis=1)), name
        # the reference's own values: NumPy's log2 is within one ulp of the correctly rounded one
        assert np.allclose(got["signal"], gold[f"{name}_sig"], rtol=4e-16, atol=1e-15), name
        same = got["signal"] == gold[f"{name}_sig"]
        assert same.mean() > 0.99
        # survival and q-values: exact given the statistic (recomputed from this run's statistic with the host classes)
        want_p = np.array([nulls[int(b)].survival(s) for b, s in zip(binned, got["signal"])])
        assert np.array_equal(got["pvals"], want_p), name
        assert np.array_equal(got["qvals"], stats.false_discovery_control(want_p, method="bh")), name
        # ... and equal to the reference's wherever the statistic is
        assert np.array_equal(got["pvals"][same], gold[f"{name}_pvals"][same]), name
        assert np.allclose(got["qvals"], gold[f"{name}_qvals"], rtol=1e-12, atol=0.0), name
        assert got["bed6_scores"].max() <= 1000 and got["bed6_scores"].dtype.kind == "i"


def test_benjamini_hochberg_edge_cases(gpu):
    import torch
    from scipy import stats

    from rocco_amd.scores import benjamini_hochberg_device

    rng = np.random.default_rng(8)
    for m in (1, 2, 3, 1023, 1024, 1025, 70001):
        p = rng.random(m) ** 3
        p[rng.integers(0, m, size=max(1, m // 10))] = p[0]  # ties
        if m > 4:
            p[1], p[2] = 0.0, 1.0
        got = benjamini_hochberg_device(torch.from_numpy(p).to(gpu)).cpu().numpy()
        assert np.array_equal(got, np.atleast_1d(stats.false_discovery_control(p, method="bh"))), m


def test_empirical_null_and_single_peak_helper(gpu):
    from rocco_amd.scores import EmpiricalNull, _peak_signal_stat

    null = EmpiricalNull([3.0, 1.0, 2.0, 2.0])
    assert null.survival(2.0) == (4 - 1 + 1.0) / 5.0 and null.survival(10.0) == 1.0 / 5.0 and null.evaluate(2.0) == 0.75
    assert np.array_equal(null.survival(np.array([0.0, 2.5])), np.array([1.0, 2.0 / 5.0]))
    with pytest.raises(ValueError):
        EmpiricalNull([])
    vals = np.array([10.0, 0.0, 35.5, 7.25])
    want = np.percentile(log2_correctly_rounded(np.maximum(vals * (1000.0 / 250.0) + 1.0, 1.0)), 75.0)
    assert _peak_signal_stat(vals, 250) == want


# ---- off the defaults --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", E.KINDS)
def test_signal_statistic_over_percentiles_pseudocounts_and_row_scales(gpu, kind):
    import torch

    from rocco_amd.scores import peak_signal_stat_device

    compared = 0
    for case in E.shape_cases():
        if case["kind"] != kind:
            continue
        counts, lengths = E.inputs(case)
        counts_t, lengths_t = torch.from_numpy(counts.copy()).to(gpu), torch.from_numpy(lengths.copy()).to(gpu)
        for pc, row_scale in E.parameters(case):
            want = E.expected_signal(case, pc, row_scale)
            got = torch.stack([peak_signal_stat_device(counts_t, lengths_t, row_scale, pc, percentile)
                               for percentile in E.PERCENTILES]).cpu().numpy()
            for i, percentile in enumerate(E.PERCENTILES):
                assert E.same_values(got[i], want[i]), (case, pc, row_scale, percentile)
            compared += want.size
    assert compared == 155672  # every case of the kind, every (pc, row scale) of it, every percentile, every row


def test_single_peak_helper_over_the_same_cases(gpu):
    from rocco_amd.scores import _peak_signal_stat

    cases = E.shape_cases()
    for index in E.FIXTURE_CASES:
        case = cases[index]
        counts, lengths = E.inputs(case)
        for j, (pc, row_scale) in enumerate(E.parameters(case)):
            want = E.expected_signal(case, pc, row_scale)
            row = (index + j) % case["P"]
            for i, percentile in enumerate(E.PERCENTILES):
                got = _peak_signal_stat(counts[row], lengths[row], row_scale=row_scale, pc=pc, percentile=percentile)
                assert isinstance(got, float) and E.same_values([got], [want[i, row]]), (case, row, pc, row_scale, percentile)


def survival_device(gpu, stat, bins, nulls):
    """rocco_hip_ecdf_survival_f64 itself: `nulls` a list of SORTED arrays, `bins[p]` an index into it."""
    import torch

    from rocco_amd import _native
    from rocco_amd import dp

    offsets = np.concatenate([[0], np.cumsum([v.size for v in nulls])]).astype(np.int64)
    stat_t = torch.from_numpy(np.ascontiguousarray(stat, dtype=np.float64)).to(gpu)
    bin_t = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.int32)).to(gpu)
    null_t, off_t = torch.from_numpy(np.concatenate(nulls)).to(gpu), torch.from_numpy(offsets).to(gpu)
    assert 0 <= int(np.min(bins)) and int(np.max(bins)) < len(nulls) and stat_t.shape == bin_t.shape
    out = torch.empty_like(stat_t)
    _native.check(_native.load().rocco_hip_ecdf_survival_f64(
        _native.solver_for(gpu.index).handle, stat_t.data_ptr(), bin_t.data_ptr(), null_t.data_ptr(), off_t.data_ptr(),
        int(stat_t.shape[0]), out.data_ptr(), dp._stream_ptr(stat_t)), "rocco_hip_ecdf_survival_f64")
    return out.cpu().numpy()


def test_survival_kernel_on_nan_infinite_and_tied_statistics(gpu):
    from rocco_amd.scores import EmpiricalNull

    named = E.survival_cases()
    models = [EmpiricalNull(null) for _, null, _ in named]
    assert [m.size for m in models[:3]] == [1, 2, 2] and max(m.size for m in models) > 200
    # one bin at a time ...
    for b, (name, _, stat) in enumerate(named):
        got = survival_device(gpu, stat, np.zeros(stat.size, dtype=np.int32), [models[b].values])
        assert np.array_equal(got, models[b].survival(stat)), name
    # ... and all bins in one launch, every statistic against every bin, over more than one block
    stat = np.concatenate([stat for _, _, stat in named])
    stat_all, bins_all = np.tile(stat, len(named)), np.repeat(np.arange(len(named)), stat.size)
    assert stat_all.size > 2 * 256 and stat_all.size % 256 != 0
    want = np.concatenate([m.survival(stat) for m in models])
    assert np.isnan(stat_all).sum() >= len(named) and not np.isnan(want).any()
    assert np.array_equal(survival_device(gpu, stat_all, bins_all, [m.values for m in models]), want)


def test_score_peak_counts_on_edge_statistics_and_unsorted_bin_keys(gpu):
    """The statistics reach the survival kernel through `score_peak_counts`: NaN (from a NaN count, and from
    -inf - -inf at pc = 0), +inf, -inf, below and above every null value, exactly on a repeated null value; a bin of
    one value; the bins' dictionary built in an order that is not the keys' order."""
    from rocco_amd.scores import EmpiricalNull, score_peak_counts

    gen = np.random.default_rng(77)
    null_values = {4000: np.concatenate([np.round(gen.gamma(2.0, 1.2, size=300), 1), [2.0, 2.0, 2.0]]),
                   100: np.array([2.0]),
                   900: np.array([5.0, 2.0, 2.0, -np.inf])}
    assert list(null_values) != sorted(null_values)
    # length 1000 at row scale 1000: a transformed count is log2(count + pc).  Four samples: the 75th percentile lies a
    # quarter of the way from the third to the fourth order statistic (+inf when the fourth is); two samples: three
    # quarters of the way from the first to the second (-inf when the first is)
    small = 4.0 + 2.0 ** -50
    four = np.array([[np.nan, 1, 1, 1], [1, 1, 1, np.inf], [0, 0, 0, 5], [0, 0, 0, 0], [3, 3, 3, 3], [4, 4, 4, 4],
                     [1e300] * 4, [small] * 4, [1, 0, 2, 1], [-np.inf, 7, 7, 7]])
    two = np.array([[1, np.nan], [0, 5], [0, 0], [3, 3], [4, 4], [1e300, 1e300], [small, small], [2, 1], [5, np.inf]])
    models = {k: EmpiricalNull(v) for k, v in null_values.items()}
    seen = []
    for per_bin in (four, two):
        counts = np.tile(per_bin, (3, 1))
        binned = np.repeat([4000, 100, 900], per_bin.shape[0])
        lengths = np.full(counts.shape[0], 1000.0)
        for pc in (0.0, 1.0):
            want_sig = E.signal(counts, lengths, 1000.0, pc, 75.0)
            want_p = E.survival(want_sig, binned, null_values)
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)  # (the narrowPeak columns of a NaN statistic)
                got = score_peak_counts(counts, lengths, binned, models, pc=pc)
                got_plain = score_peak_counts(counts, lengths, binned, null_values, pc=pc)  # the values themselves, unsorted
            assert E.same_values(got["signal"], want_sig), pc
            assert np.array_equal(got["pvals"], want_p) and np.array_equal(got_plain["pvals"], want_p), pc
            assert np.array_equal(got["pvals"], np.array([models[int(b)].survival(x) for b, x in zip(binned, want_sig)])), pc
            assert np.array_equal(got["qvals"], E.bh(want_p)), pc
            seen.append(want_sig[:per_bin.shape[0]])
    four_0, four_1, two_0, two_1 = seen
    assert np.isnan(four_0[0]) and np.isnan(two_1[0])                       # from a NaN count
    assert np.isnan(four_0[3]) and np.isnan(two_0[2])                       # -inf - -inf, from finite counts
    assert four_0[1] == np.inf and four_1[1] == np.inf and two_0[1] == -np.inf
    assert four_1[4] == 2.0 and four_0[5] == 2.0 and two_1[3] == 2.0 and two_0[4] == 2.0  # on the repeated null value
    assert 2.0 < four_0[7] < 2.0 + 1e-15 and four_1[3] == 0.0 and four_0[6] > 900.0      # just above it; below / above all


@pytest.mark.parametrize("m", E.BH_SIZES)
def test_benjamini_hochberg_ties_zeros_and_invalid_values(gpu, m):
    import torch

    from rocco_amd.scores import benjamini_hochberg_device

    for name, p in E.bh_vectors(m).items():
        got = benjamini_hochberg_device(torch.from_numpy(p.copy()).to(gpu)).cpu().numpy()
        assert np.array_equal(got, E.bh(p)), (m, name)  # (== : the sign of a zero is nobody's contract)
    for p in E.bh_invalid_vectors(m):
        with pytest.raises(ValueError) as info:
            benjamini_hochberg_device(torch.from_numpy(p.copy()).to(gpu))
        assert str(info.value) == E.BH_ERROR, (m, p)


def test_benjamini_hochberg_negative_zero_is_a_zero(gpu):
    import torch

    from rocco_amd.scores import benjamini_hochberg_device

    got = benjamini_hochberg_device(torch.tensor([0.2, -0.0, 0.5], dtype=torch.float64, device=gpu)).cpu().numpy()
    assert np.array_equal(got, E.bh([0.2, -0.0, 0.5])) and got[0] > 0.25 and got[2] == 0.5


def test_score_peak_counts_without_pseudocount_on_mostly_zero_counts(gpu):
    """pc = 0 on integer counts that are mostly zero: statistics that are -inf and NaN (inf - inf in the interpolation)
    from finite counts, through the survival (nulls that hold -inf and NaN themselves) and Benjamini-Hochberg."""
    from rocco_amd.scores import EmpiricalNull, _assign_length_bins, score_peak_counts

    seen = dict(cases=0, nan=0, minus_inf=0, finite=0, null_nan=0, null_minus_inf=0, single=0)
    for case in E.shape_cases():
        if case["kind"] != "mostly_zero" or case["P"] < 255 or case["K"] < 2:
            continue
        counts, _ = E.inputs(case)
        gen = np.random.default_rng([case["index"], 5])
        lengths = gen.integers(50, 4000, size=case["P"]).astype(np.float64)
        binned, representatives = _assign_length_bins(lengths, max_bins=24)
        # nulls as `get_ecdf` would find them at pc = 0: the same statistic of random mostly-zero rows
        nulls = {}
        for i, r in enumerate(representatives):
            shape = (1 if i == 0 else int(gen.integers(2, 300)), case["K"])
            rows = gen.integers(0, 6, size=shape) * (gen.random(shape) < 0.4)
            nulls[int(r)] = E.signal(rows.astype(np.float64), np.full(shape[0], float(r)), 1000.0, 0.0, 75.0)
        want_sig = E.signal(counts, lengths, 1000.0, 0.0, 75.0)
        want_p = E.survival(want_sig, binned, nulls)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)  # (the narrowPeak columns of NaN and -inf statistics)
            got = score_peak_counts(counts, lengths, binned, {k: EmpiricalNull(v) for k, v in nulls.items()}, pc=0.0)
        assert E.same_values(got["signal"], want_sig), case
        assert np.array_equal(got["pvals"], want_p), case
        assert np.array_equal(got["qvals"], E.bh(want_p)), case
        seen["cases"] += 1
        seen["nan"] += int(np.isnan(want_sig).sum())
        seen["minus_inf"] += int((want_sig == -np.inf).sum())
        seen["finite"] += int(np.isfinite(want_sig).sum())
        seen["null_nan"] += sum(int(np.isnan(v).sum()) for v in nulls.values())
        seen["null_minus_inf"] += sum(int((v == -np.inf).sum()) for v in nulls.values())
        seen["single"] += sum(v.size == 1 for v in nulls.values())
    assert seen["cases"] == 7 and min(seen.values()) > 0, seen
