"""tests/wls_trend_cases.py without a GPU: the cases of tests/test_gpu_wls_trend_edges.py have the structure they claim
(computed here from |x| and the variances the scoring will see, y', alone), the oracle's trend fit on them equals an
independent NumPy restatement bit for bit, and the oracle's given-variances entry fed the oracle's own rolling variances is
the oracle's `score_centered_wls`."""
import numpy as np
import pytest

import wls_trend_cases as tc
from test_wls_oracle import reference_backend_cases


def seen(case):
    m, V, kw = case[:3]
    return tc.seen_variances(V, m.shape[1], kw["spatial_window"])


def test_shape_facts():
    """Bins, widths and even-width bins of the sizes the cases use; which values share a cell."""
    facts = {4096: (13, {315, 316}, [12]), 4099: (13, {315, 316}, [3, 6, 9, 12]),
             70001: (17, {4117, 4118}, [1, 2, 4, 5, 7, 8, 9, 11, 12, 14, 15, 16]),
             150001: (18, {8333, 8334}, [2, 5, 7, 10, 12, 15, 17])}
    for n, (bins, widths, even) in facts.items():
        e = tc.bin_edges(n)
        assert tc.trend_bins(n) == bins == len(e) - 1 and e[0] == 0 and e[-1] == n
        assert {e[b + 1] - e[b] for b in range(bins)} == widths, n
        assert tc.even_bins(n) == even, n
    # n + 1 a power of two: the bins expression takes the logarithm's own rounding
    assert [tc.trend_bins(n) for n in (4095, 8191, 65535)] == [13, 14, 17]
    assert tc.even_bins(4095) == [] and tc.even_bins(65535) == []
    assert tc.EVEN in tc.even_bins(tc.N) and tc.ODD not in tc.even_bins(tc.N)
    assert {tc.WIDE_EVEN, tc.WIDE_EVEN2} <= set(tc.even_bins(tc.N_WIDE)) and tc.WIDE_ODD not in tc.even_bins(tc.N_WIDE)
    assert all(w > tc.SELECT_CHUNK for w in facts[150001][1]) and all(w <= tc.SELECT_CHUNK for w in facts[70001][1])
    # 4097 distinct values BASE (1 + j 2^-40) share one cell, and so do 5000 consecutive bit patterns from BASE
    v = tc.in_cell(np.arange(4097))
    assert np.unique(v).size == 4097 and np.unique(tc.cells(v)).size == 1 and v[0] == tc.BASE and np.all(np.diff(v) > 0)
    c = (tc.keys(np.array([tc.BASE]))[0] + np.arange(5000, dtype=np.uint64)).view(np.float64)
    assert np.unique(tc.cells(c)).size == 1 and tc.cells(c)[0] == tc.cells(v)[0]
    w = tc.craft_low_bits(4118, None)
    assert np.all(np.diff(tc.keys(w)) == 1) and tc.cells(w)[0] == tc.cells(v)[0]
    assert [tc.padded(c) for c in (1, 64, 65, 128, 4095, 4096)] == [64, 64, 128, 128, 4096, 4096]
    # the floored inputs: one value behind the floor; the next double is not
    low = np.maximum(np.array(tc.FLOORED_INPUTS), tc.FLOOR)
    assert np.all(low == tc.FLOOR) and np.nextafter(tc.FLOOR, 1.0) > tc.FLOOR
    assert tc.cells(np.array([np.nextafter(tc.FLOOR, 1.0)]))[0] == tc.cells(np.array([tc.FLOOR]))[0]


def test_cases_are_listed_once_and_deterministic():
    assert len(set(tc.NAMES)) == len(tc.NAMES) == 24
    for name in ("cell_4096", "boundary_tie", "many_segments"):
        again = tc.BUILDERS[name]()
        got = tc.case(name)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), name


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_has_the_structure_it_claims(name):
    m, V, kw, expected_sorted, claims = tc.case(name)
    K, n = m.shape
    window = kw["spatial_window"]
    assert (K, n, window) == (claims["K"], claims["n"], claims["window"]) and window % 2 == 1
    assert V.shape == (K, n - window + 1) and m.dtype == V.dtype == np.float64
    assert claims["bins"] == tc.trend_bins(n)
    y = seen(tc.case(name))
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(y)) and np.all(y >= tc.FLOOR)
    if claims["x_distinct"]:
        for k in range(K):
            assert np.unique(np.abs(m[k])).size == n, (name, k)
    assert expected_sorted == (K if n < tc.SELECT_MIN else (1 if name == "boundary_tie" else 0))
    for row, b, expect in claims["bin"]:
        got = tc.census(m[row], y[row], b)
        for key, want in expect.items():
            assert got[key] == want, (name, row, b, key, got[key], want)
    assert claims["bin"] or name in ("shapes_of_the_fit", "many_segments")


def one(name, row, b):
    m, _V, _kw, _s, _c = tc.case(name)
    return tc.census(m[row], seen(tc.case(name))[row], b)


def test_cases_reach_the_branches_they_are_named_for():
    """The claims in the kernel's terms: which cells are gathered and sorted and which are counted out, where the upper middle
    value comes from, which rule of the finish kernel decides."""
    e, o = tc.EVEN, tc.ODD
    half_even, half_odd = 4118 // 2, 4117 // 2
    # the threshold between the two paths, with distinct values: count_le == rank + 1 on both sides of it
    for name, count in (("cell_4096", 4096), ("cell_4097", 4097)):
        for row, b, w in ((0, e, 4118), (2, o, 4117)):
            c = one(name, row, b)
            assert c["width"] == w and c["cell_count"] == count and c["cell_distinct"] and c["count_le"] == c["rank"] + 1
            assert w - count in (21, 22, 20) and 0 < c["rank_in_cell"] < count - 1
    assert one("cell_4096", 0, e)["cell_count"] == tc.CELL_MAX == one("cell_4096", 0, e)["padded"]
    assert one("cell_4097", 0, e)["cell_count"] == tc.CELL_MAX + 1
    # padding steps 64, 64, 128; a cell of one value has its upper middle value in a higher cell
    assert [one(n_, 0, e)["padded"] for n_ in ("cell_1", "cell_64", "cell_65")] == [64, 64, 128]
    assert [one(n_, 0, e)["cell_count"] for n_ in ("cell_1", "cell_64", "cell_65")] == [1, 64, 65]
    c = one("cell_1", 0, e)
    assert c["even"] and not c["upper_in_cell"] and c["upper"] > c["lower"]
    # rank + 1 < count false | true at the cell's first value
    c = one("median_last_of_cell", 0, e)
    assert c["even"] and c["lower_is_cell_max"] and c["rank_in_cell"] + 1 == c["cell_count"] == 200 and c["upper_far"]
    assert not c["upper_in_cell"]
    c = one("median_first_of_cell", 0, e)
    assert c["even"] and c["lower_is_cell_min"] and c["rank_in_cell"] == 0 and c["upper_in_cell"] and c["upper"] > c["lower"]
    # runs: count_le == w/2 (the upper value is the next distinct one) | count_le >= w/2 + 1 (the run's value)
    for name, wide, counted in (("run_to_the_middle_long", True, True), ("run_to_the_middle_short", False, False),
                                ("window_31", False, False), ("window_63", False, False)):
        c = one(name, 0, tc.WIDE_EVEN if wide else e)
        assert c["even"] and c["count_le"] == c["width"] // 2 and c["upper"] == float(tc.in_cell(1)) > c["lower"] == tc.BASE
        assert (c["run"] > tc.CELL_MAX and c["cell_count"] > tc.CELL_MAX) if counted else (c["run"] < 1000 and c["cell_count"] < 1000)
        c = one(name, 2, tc.WIDE_ODD if wide else o)
        assert not c["even"] and c["run_last"] == c["rank"] and c["lower"] == tc.BASE
    for name, wide, counted in (("run_past_the_middle_long", True, True), ("run_past_the_middle_short", False, False)):
        c = one(name, 0, tc.WIDE_EVEN if wide else e)
        assert c["even"] and c["count_le"] >= c["width"] // 2 + 1 and c["upper"] == c["lower"] == tc.BASE
        assert c["run_first"] < c["rank"] and ((c["run"] > tc.CELL_MAX) if counted else (c["run"] < 1000 and c["cell_count"] < 1000))
    assert half_even == one("run_to_the_middle_short", 0, e)["count_le"] and half_odd == one("run_to_the_middle_short", 2, o)["rank"]
    # the floor: one run of 1e-8 over both middle ranks (row 0), ending at the median (row 2)
    c = one("floored", 0, e)
    assert c["lower"] == c["upper"] == tc.FLOOR and c["run_first"] == 0 and c["count_le"] > half_even + 1
    V0 = tc.case("floored")[1]
    for special in tc.FLOORED_INPUTS + (float(np.nextafter(tc.FLOOR, 1.0)),):
        assert np.any(V0[0].view(np.uint64) == np.array([special]).view(np.uint64)[0]), special
    c = one("floored", 2, o)
    assert c["lower"] == tc.FLOOR and c["run_last"] == c["rank"]
    # every digit but the last two shared (counted out: more than CELL_MAX values) | first digits spread over the range
    c = one("low_bits_only", 0, e)
    assert c["cell_count"] == c["width"] > tc.CELL_MAX and c["distinct"] == c["width"] and 9 < c["shared_high_bits"] <= 20
    c = one("full_range", 0, e)
    assert c["first_digits"] > 500 and c["cell_count"] < 64
    s = np.sort(seen(tc.case("full_range"))[0][np.argsort(np.abs(tc.case("full_range")[0][0]))][70001 * e // 17:70001 * (e + 1) // 17])
    assert s[0] == 1.0e-8 and s[-1] == 1.0e300
    # two chunks per segment, with a full gathered cell and a counted run in one row
    c5, c10 = one("wide_segments", 0, tc.WIDE_EVEN), one("wide_segments", 0, tc.WIDE_EVEN2)
    assert c5["chunks"] == c10["chunks"] == 2 and c5["cell_count"] == tc.CELL_MAX and c10["run"] > tc.CELL_MAX
    assert c10["count_le"] == c10["width"] // 2 and tc.case("wide_segments")[0].shape == (2, 150001)


def test_shapes_of_the_fit_and_many_segments():
    m, _V, _kw, _s, claims = tc.case("shapes_of_the_fit")
    y = seen(tc.case("shapes_of_the_fit"))
    assert m.shape == (4, 70001) and claims["medians"] == ["increasing", "decreasing", "sawtooth", "equal"]
    d = [np.diff(tc.bin_medians(m[k], y[k])) for k in range(4)]
    assert np.all(d[0] > 0) and np.all(d[1] < 0) and np.all(d[3] == 0)
    assert np.all(d[2][0::2] > 0) and np.all(d[2][1::2] < 0)
    m, _V, _kw, _s, claims = tc.case("many_segments")
    y = seen(tc.case("many_segments"))
    K, n = m.shape
    assert (K, n) == (33, 4099) and K * tc.trend_bins(n) == claims["segments"] == 429
    for k in range(K):
        levels = np.unique(y[k]).size
        assert (levels > 4000) if k == claims["plain_row"] else (levels == claims["levels"] == 3)
    for b in range(13):
        c = tc.census(m[0], y[0], b)
        assert c["cell_count"] == c["run"] <= 316  # runs in small cells: settled from the gathered cell


def test_boundary_tie_rows():
    m, _V, _kw, expected_sorted, claims = tc.case("boundary_tie")
    n = m.shape[1]
    e = tc.bin_edges(n)
    row, b = claims["tie_boundary"]
    x = np.sort(np.abs(m[row]))
    ties = np.flatnonzero(np.diff(x) == 0)
    assert ties.tolist() == [e[b] - 1] and expected_sorted == 1
    row, pairs = claims["inner_pairs"]
    x = np.sort(np.abs(m[row]))
    ties = np.flatnonzero(np.diff(x) == 0)
    assert ties.size == pairs == 7 and all(r + 1 not in e and r not in e and r + 2 not in e for r in ties.tolist())
    assert np.unique(np.abs(m[2])).size == n


# ---- the oracle's trend fit against a NumPy restatement --------------------------------------------------------------------------

def numpy_trend(x_row, y_row):
    """wls_backend.c:394-608 for n >= 4 and finite inputs: pairs by (x, y), equal-count bins, their medians, pooled adjacent
    violators, knots, linear interpolation."""
    x, y = np.abs(x_row), np.maximum(y_row, 1.0e-8)
    n = x.shape[0]
    order = np.lexsort((y, x))
    xs, ys = x[order], y[order]
    bins = int(max(4.0, np.floor(1.0 + np.log(n + 1.0) / np.log(2.0))))
    blocks = []  # [value, weight, [median x of every bin pooled into the block]]
    for b in range(bins):
        left, right = (b * n) // bins, ((b + 1) * n) // bins
        if right <= left:
            continue
        blocks.append([float(np.median(ys[left:right])), max(float(right - left), 1.0e-8), [float(np.median(xs[left:right]))]])
        while len(blocks) >= 2 and blocks[-2][0] > blocks[-1][0]:
            (v1, w1, c1), (v2, w2, c2) = blocks[-2], blocks[-1]
            blocks[-2:] = [[((v1 * w1) + (v2 * w2)) / (w1 + w2), w1 + w2, c1 + c2]]
    kc, kv = [], []
    for value, _w, centres in blocks:
        for c in centres:
            vv = max(value, 1.0e-8)
            if kc and c <= kc[-1]:
                kv[-1] = max(kv[-1], vv)
            else:
                kc.append(c)
                kv.append(vv)
    kc, kv = np.array(kc), np.array(kv)
    if kc.size == 1:
        return np.full(n, max(kv[0], 1.0e-8))
    left = np.clip(np.searchsorted(kc, x, side="right") - 1, 0, kc.size - 2)
    w = (x - kc[left]) / (kc[left + 1] - kc[left])
    out = kv[left] + (w * (kv[left + 1] - kv[left]))
    out = np.where(x <= kc[0], kv[0], np.where(x >= kc[-1], kv[-1], out))
    return np.maximum(out, 1.0e-8)


@pytest.mark.parametrize("name", tc.NAMES)
def test_oracle_trend_equals_the_numpy_restatement(oracle, name):
    m, _V, _kw, _s, claims = tc.case(name)
    y = seen(tc.case(name))
    rows = sorted({row for row, _b, _e in claims["bin"]} | {0, 1}) if m.shape[0] <= 4 else [0, 16, 17, 32]
    if name in ("shapes_of_the_fit", "boundary_tie"):
        rows = list(range(m.shape[0]))
    for row in rows:
        got = oracle.monotone_variance_trend(m[row], y[row])
        assert got.tobytes() == numpy_trend(m[row], y[row]).tobytes(), (name, row)


def test_given_variances_oracle_is_the_oracle_on_its_own_variances(oracle):
    rng = np.random.default_rng(23)
    cases = list(reference_backend_cases())
    cases.append(("n=4096 K=3", np.round(rng.normal(0, 1, (3, 4096)), 2)))
    cases.append(("n=70001 K=2", rng.normal(0, 1, (2, 70001)) * np.exp(rng.normal(0, 0.5, (1, 70001)))))
    for name, m in cases:
        for kw in ({}, {"spatial_window": 5, "min_effect": 0.25}, {"spatial_window": 63, "prior_df": 0.0, "precision_floor_ratio": 0.5}):
            window = oracle.wls_spatial_window(m.shape[1], kw.get("spatial_window", 31))
            starts = oracle.rolling_variances_at_starts(m, kw.get("spatial_window", 31))
            want = oracle.score_centered_wls(m, **kw)
            if window == 0:
                assert starts is None and m.shape[1] < 5 and want[7] == 0, name
                continue
            assert starts.shape == (m.shape[0], m.shape[1] - window + 1) and want[7] == window, name
            got = oracle.score_centered_wls(m, variances=starts, **kw)
            for g, w in zip(got[:6], want[:6]):
                assert g.tobytes() == w.tobytes(), (name, kw)
            assert got[6:] == want[6:]
            # not a function that ignores what it is given
            other = oracle.score_centered_wls(m, variances=starts * 1.5 + 0.25, **kw)
            assert other[2].tobytes() != want[2].tobytes(), (name, kw)
    with pytest.raises(ValueError):
        oracle.score_centered_wls(np.zeros((2, 100)), variances=np.zeros((2, 100)))
