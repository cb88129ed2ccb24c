"""Host side of the locus-axis summaries (no GPU): the rank np.quantile(..., method="higher") picks, the
two-order-statistic form of the null scale and the p <= sorted[cutoff] form of the Benjamini-Hochberg mask against the
reference's recorded outputs with NumPy standing in for the device calls, the string, the signatures and the errors that
need no device."""
import inspect
import json

import numpy as np
import pytest

from locus_summaries_cases import DEFAULT_QUANTILES, NumpyVector, cases, errors, golden, same_bits, same_float

LARGE = (934387, 1000003, 4979129, 4979130, 5000001)


def test_the_functions_are_exported_under_the_reference_names():
    import rocco_amd

    for name in ("cscores_quantiles", "benjamini_hochberg", "candidate_mask_from_wls", "_standardize_wls_z_scores", "_robust_scale",
                 "cscores_quantiles_batch_device", "benjamini_hochberg_device", "candidate_mask_from_wls_device",
                 "_standardize_wls_z_scores_device", "_robust_scale_device"):
        assert callable(getattr(rocco_amd, name)), name
    import rocco_amd.inference as inference
    import rocco_amd.rocco as rocco

    assert rocco_amd.cscores_quantiles is rocco.cscores_quantiles
    assert rocco_amd.benjamini_hochberg is inference.benjamini_hochberg


def test_signatures_and_defaults_are_the_references():
    import rocco_amd.inference as inference
    import rocco_amd.rocco as rocco

    recorded = json.loads(str(golden()["signatures"]))
    assert set(recorded) == {"cscores_quantiles", "_robust_scale", "benjamini_hochberg", "_standardize_wls_z_scores",
                             "candidate_mask_from_wls"}
    for name, text in recorded.items():
        fn = getattr(rocco if name == "cscores_quantiles" else inference, name)
        assert str(inspect.signature(fn)) == text, name


def test_rank_is_what_np_quantile_higher_picks_small_lengths():
    from rocco_amd.rocco import _higher_quantile_rank

    q = np.array(DEFAULT_QUANTILES)
    for n in range(1, 3000):
        want = np.quantile(np.arange(n), q, method="higher")
        assert [_higher_quantile_rank(n, v) for v in q] == [int(w) for w in want], n


@pytest.mark.parametrize("n", LARGE)
def test_rank_is_what_np_quantile_higher_picks_chromosome_lengths(n):
    from rocco_amd.rocco import _higher_quantile_rank

    q = np.array(DEFAULT_QUANTILES)
    want = np.quantile(np.arange(n), q, method="higher")
    assert [_higher_quantile_rank(n, v) for v in q] == [int(w) for w in want]


def test_quantile_errors_are_numpys_in_the_references_order():
    from rocco_amd.rocco import _check_quantiles

    recorded = errors("cscores_quantiles")
    assert len(recorded) == 3
    for entry in recorded:
        n = 0 if entry["input"] == "empty" else 10
        quantiles = entry["kwargs"].get("quantiles", DEFAULT_QUANTILES)
        with pytest.raises(Exception) as caught:
            _check_quantiles(n, quantiles)
        assert type(caught.value).__name__ == entry["class"] and str(caught.value) == entry["text"]
    _check_quantiles(10, DEFAULT_QUANTILES)
    _check_quantiles(1, [0.3, 0.25, 0.3])


def test_the_string_is_the_references_given_the_recorded_values():
    from rocco_amd.rocco import _format_quantiles

    same_numpy = str(golden()["numpy_version"]).split(".")[0] == np.__version__.split(".")[0]
    for i, case in enumerate(cases("quantile_cases")):
        quantiles = case["quantiles"] if case["quantiles"] is not None else np.array(DEFAULT_QUANTILES)
        text = _format_quantiles(list(quantiles), list(golden()[f"quantile_values_{i}"]), case["add_newlines"])
        assert text.startswith("\n") == case["add_newlines"] and text.endswith("\n") == case["add_newlines"]
        if same_numpy:  # (the repr of np.float64 inside the dict is NumPy >= 2's)
            assert text == case["text"], case


def test_quantile_values_by_rank_equal_the_recorded_ones():
    """the rank rule and the NaN rule on the fixture itself, np.sort standing in for the select"""
    from rocco_amd.rocco import _higher_quantile_rank

    for i, case in enumerate(cases("quantile_cases")):
        scores = golden()[f"scores_{case['scores']}"]
        quantiles = case["quantiles"] if case["quantiles"] is not None else DEFAULT_QUANTILES
        vec = NumpyVector(scores)
        got = vec.select([_higher_quantile_rank(vec.n, q) for q in quantiles])
        if vec.counts()[0] > 0:
            got = [float("nan")] * len(got)
        want = golden()[f"quantile_values_{i}"]
        assert all(same_float(g, w) for g, w in zip(got, want)), case


def test_null_scale_from_two_order_statistics_is_the_references():
    from rocco_amd.inference import _null_scale_of

    seen = set()
    for i, case in enumerate(cases("mask_cases")):
        vec = NumpyVector(golden()[f"z_{case['z']}"])
        null_scale = _null_scale_of(vec)
        assert same_bits(null_scale, case["null_scale"]), case
        if case["z"] not in seen:
            seen.add(case["z"])
            assert same_bits(vec.divide_finite(max(null_scale, 1.0e-6)), golden()[f"standardized_{case['z']}"]), case
        mask = vec.threshold_mask(max(null_scale, 1.0e-6), case["tail_z"], case["min_signal"], case["min_signal"] > 0)
        assert np.array_equal(mask, golden()[f"mask_{i}"]), case
    assert {"positive_odd", "positive_even", "positive_with_minus_inf", "non_finite", "one_negative"} <= seen


def test_null_scale_refuses_a_vector_without_finite_values():
    from rocco_amd.inference import _null_scale_of

    text = errors("_standardize_wls_z_scores")[0]["text"]
    for values in ([np.nan, np.inf, -np.inf], []):
        with pytest.raises(ValueError) as caught:
            _null_scale_of(NumpyVector(values))
        assert str(caught.value) == text


def test_robust_scale_from_two_selects_is_the_references():
    from rocco_amd.inference import _robust_scale_of

    for case in cases("scale_cases"):
        got = _robust_scale_of(NumpyVector(golden()[f"values_{case['values']}"]), case["floor"])
        assert isinstance(got, float) and same_float(got, case["result"]), (case, got)


def test_bh_mask_as_at_most_the_cutoff_value_is_the_references():
    from rocco_amd.inference import _bh_mask_of

    nonempty = 0
    for i, case in enumerate(cases("bh_cases")):
        p = golden()[f"p_{case['p']}"]
        mask = _bh_mask_of(NumpyVector(p), case["fdr"])
        mask = np.zeros(p.shape[0], dtype=bool) if mask is None else mask
        assert np.array_equal(mask, golden()[f"bh_mask_{i}"]) and int(mask.sum()) == case["passing"], case
        nonempty += case["passing"] > 0
    assert nonempty >= 20
    # the case a sort of bit patterns gets wrong unless the sign-set NaN in front is stepped over: nothing passes
    tricky = [(i, c) for i, c in enumerate(cases("bh_cases")) if c["p"] == "minus_nan_at_cutoff" and c["fdr"] == 0.05]
    assert len(tricky) == 1 and tricky[0][1]["passing"] == 0 and np.signbit(golden()["p_minus_nan_at_cutoff"][0])


def test_errors_and_early_returns_that_need_no_device():
    import rocco_amd

    functions = {"benjamini_hochberg": rocco_amd.benjamini_hochberg, "_standardize_wls_z_scores": rocco_amd._standardize_wls_z_scores,
                 "candidate_mask_from_wls": rocco_amd.candidate_mask_from_wls}
    inputs = {"two_dimensional": np.zeros((2, 3)), "all_non_finite": np.array([np.nan, np.inf, -np.inf]), "empty": np.zeros(0)}
    checked = 0
    for entry in cases("errors"):
        if entry["function"] in functions:
            with pytest.raises(Exception) as caught:
                functions[entry["function"]](inputs[entry["input"]])
            assert type(caught.value).__name__ == entry["class"] and str(caught.value) == entry["text"], entry
            checked += 1
    assert checked == 6
    empty = rocco_amd.benjamini_hochberg(np.zeros(0))
    assert empty.dtype == np.bool_ and empty.shape == (0,)
    assert rocco_amd._robust_scale(np.zeros(0)) == 1.0e-6 and rocco_amd._robust_scale(np.zeros(0), floor=0.5) == 0.5
