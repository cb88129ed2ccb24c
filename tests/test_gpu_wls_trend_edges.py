"""GPU: the y side of the sort-free trend fit (rocco_amd/csrc/wls.hip, wls_deal_kernel .. wls_knots_rows_kernel) on DICTATED
local variances -- the cases of tests/wls_trend_cases.py, whose structure tests/test_wls_trend_cases_host.py asserts on the
CPU -- through `score_centered_wls_device(..., variances_t=)` against the oracle's given-variances entry: six tracks bit for
bit, and the number of rows that took the sorted path (a fallback must not hide a failure of the select path).  With them:
the batched rolling launch against the oracle's per-start variances, the kernel of rows under 5 loci, and what the
given-variances entry refuses."""
import numpy as np
import pytest

import wls_trend_cases as tc

pytestmark = pytest.mark.gpu
ORDER = ("scores", "mean", "raw", "prior", "mod", "se")


def on_device(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()  # (a copy: the cases are read-only)


@pytest.mark.parametrize("name", tc.NAMES)
def test_dictated_variances_match_oracle(gpu, oracle, name):
    from rocco_amd.inference import score_centered_wls_device, wls_sorted_rows

    m, V, kw, expected_sorted, _claims = tc.case(name)
    got = score_centered_wls_device(on_device(m), variances_t=on_device(V), **kw)
    sorted_rows = wls_sorted_rows()
    want = oracle.score_centered_wls(m, variances=V, **kw)
    for label, g, w in zip(ORDER, got[:6], want[:6]):
        assert g.cpu().numpy().tobytes() == w.tobytes(), (name, label)
    assert got[6:] == want[6:], name
    assert sorted_rows == expected_sorted, name


# ---- the batched rolling launch ----------------------------------------------------------------------------------------------------

ROLLING_N = (4, 5, 6, 31, 32, 64, 65, 511, 513, 4099)
ROLLING_K = (1, 3, 9)
_rolling = {}


def rolling_reference(oracle, window):
    """The ragged list and the oracle's per-start variances of each matrix, computed once per window."""
    if window not in _rolling:
        rng = np.random.default_rng(4242)
        mats = [np.round(rng.normal(0.0, 1.0, size=(K, n)) * np.exp(rng.normal(0.0, 0.5, size=(1, n))), 3)
                for n in ROLLING_N for K in ROLLING_K]
        _rolling[window] = (mats, [oracle.rolling_variances_at_starts(m, window) for m in mats])
    return _rolling[window]


@pytest.mark.parametrize("group", [1, 2, 4, 8])
@pytest.mark.parametrize("window", [5, 31, 63])
def test_batched_rolling_launch_matches_oracle_per_start(gpu, oracle, monkeypatch, window, group):
    from rocco_amd.inference import wls_rolling_variances_batch_device, wls_spatial_window

    monkeypatch.setenv("ROCCO_HIP_ROLLING_GROUP", str(group))
    mats, want = rolling_reference(oracle, window)
    got = wls_rolling_variances_batch_device([on_device(m) for m in mats], spatial_window=window)
    assert len(got) == len(mats) == 30
    single_start = window_is_row = 0
    for m, g, w in zip(mats, got, want):
        K, n = m.shape
        resolved = wls_spatial_window(n, window)
        assert resolved == oracle.wls_spatial_window(n, window)
        if n < 5:
            assert g is None and w is None and resolved == 0
            continue
        assert tuple(g.shape) == w.shape == (K, n - resolved + 1), (K, n, window, group)
        assert g.cpu().numpy().tobytes() == w.tobytes(), (K, n, window, group)
        single_start += n == 5
        window_is_row += resolved == n
    assert single_start == 3 and window_is_row >= 3


# ---- rows of fewer than 5 loci ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_rows_without_a_window(gpu, oracle, n, K):
    """wls_tiny_kernel: the row's robust scale for every locus (wls_backend.c:834-851)."""
    from rocco_amd.inference import score_centered_wls

    rng = np.random.default_rng(100 * n + K)
    spread = rng.normal(0.0, 2.0, size=(K, n))
    ties = np.round(spread, 0)                               # equal values inside a row
    constant = np.repeat(rng.normal(size=(K, 1)), n, axis=1)  # MAD 0
    narrow = 1.0 + 1.0e-8 * rng.normal(size=(K, n))           # 0 < 1.4826 MAD < 1e-6
    mixed = np.where((np.arange(K) % 3 == 0)[:, None], constant, np.where((np.arange(K) % 3 == 1)[:, None], narrow, spread))
    if n >= 2:
        mad = 1.4826 * np.median(np.abs(narrow - np.median(narrow, axis=1, keepdims=True)), axis=1)
        assert np.all(mad < 1.0e-6) and (n == 2 or np.any(mad > 0.0))
    for mat in (spread, ties, constant, narrow, mixed):
        for kw in ({}, {"prior_df": 0.0}, {"precision_floor_ratio": 0.5}, {"min_effect": 0.25, "lower_bound_z": 0.0},
                   {"prior_df": 0.0, "precision_floor_ratio": 0.5, "spatial_window": 5}):
            got = score_centered_wls(mat, **kw)
            want = oracle.score_centered_wls(mat, **kw)
            for label, g, w in zip(ORDER, got[:6], want[:6]):
                assert np.asarray(g).tobytes() == w.tobytes(), (n, K, kw, label)
            assert got[6:] == want[6:] and got[7] == 0


# ---- what the given-variances entry refuses ----------------------------------------------------------------------------------------

def test_given_variances_refuse_windows_above_the_tiled_limit(gpu):
    from rocco_amd.inference import score_centered_wls_device

    rng = np.random.default_rng(9)
    m = on_device(rng.normal(size=(2, 300)))
    for window in (65, 101, 10 ** 6):
        with pytest.raises(ValueError):
            score_centered_wls_device(m, spatial_window=window, variances_t=on_device(np.ones((2, 300))))
    # (63 is the largest window that takes them)
    score_centered_wls_device(m, spatial_window=63, variances_t=on_device(np.ones((2, 300 - 63 + 1))))


@pytest.mark.parametrize("n,sorted_rows", [(300, 2), (5000, 0)])
def test_given_variances_refuse_infinity(gpu, oracle, n, sorted_rows):
    """+inf among the given variances: on the sorted path (n = 300) and on the select path (n = 5000), at an inner start and at
    the two clamped ends; the same call without it passes and matches the oracle."""
    from rocco_amd.inference import score_centered_wls_device, wls_sorted_rows

    rng = np.random.default_rng(n)
    m = rng.normal(size=(2, n))
    V = 0.5 * np.exp(rng.normal(0.0, 0.7, size=(2, n - 4)))
    got = score_centered_wls_device(on_device(m), spatial_window=5, variances_t=on_device(V))
    assert wls_sorted_rows() == sorted_rows
    want = oracle.score_centered_wls(m, spatial_window=5, variances=V)
    for g, w in zip(got[:6], want[:6]):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    for row, start in ((1, n // 2), (0, 0), (1, n - 5)):
        bad = V.copy()
        bad[row, start] = np.inf
        with pytest.raises(ValueError):
            score_centered_wls_device(on_device(m), spatial_window=5, variances_t=on_device(bad))
