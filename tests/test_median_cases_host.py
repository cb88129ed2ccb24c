"""tests/median_cases.py without a GPU: the reference the GPU tests compare against is pinned by an independent statement
of the median, and the adversarial columns are what their labels say."""
import numpy as np
import pytest

import median_cases as mc

DTYPES = ("float64", "float32")


def _columns(K, dtype):
    m, labels = mc.columns(K, dtype, seed=K)
    return m, np.array(labels)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", mc.ks_for("host"))
def test_reference_median_is_the_sorted_median(K, dtype):
    m, labels = _columns(K, dtype)
    assert m.dtype == np.dtype(dtype) and m.shape == (K, len(labels)) and m.flags.c_contiguous
    assert 130 <= len(labels) <= 200 and len(labels) % 16 != 0
    message = mc.mismatch(mc.reference_median(m), mc.sorted_median(m), labels, K)
    assert message is None, message


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9])
def test_small_k_columns_are_built(K):
    m, labels = _columns(K, "float64")
    assert sorted(set(labels)) == sorted(mc.kinds_at(K))
    assert mc.mismatch(mc.reference_median(m), mc.sorted_median(m), labels, K) is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 16, 17, 64, 65, 100, 101, 199, 200, 256, 300, 301, 600, 1200, 1201])
def test_every_kind_occurs_and_no_column_is_constant_by_accident(K, dtype):
    m, labels = _columns(K, dtype)
    # the list of kinds, stated here from the issue and not read back from the module
    named = {"random": ["distinct", "ties", "counts"],
             "order": ["ascending", "descending", "organ-pipe", "valley", "rotated", "even-then-odd", "blocks64-descending",
                       "blocks100-descending"],
             "two": [f"{c}/{p}" for c in ("below-half", "half", "above-half", "above-upper-half")
                     for p in ("random", "first", "last", "alternating")],
             "inf": ["one-plus", "one-minus", "one-each", "plus-majority", "minus-majority", "both-in-block64",
                     "both-in-block100"] + (["plus-exactly-half", "half-minus-half-plus"] if K % 2 == 0 else [])
                    + (["different-block64"] if K > 64 else []) + (["different-block100"] if K > 100 else []),
             "nan": ["row-0", "row-last", "row-middle", "last-real-row", "with-plus-inf", "with-minus-inf", "all"]
                    + (["row-multiple-64-or-100", "two-different-blocks"] if K > 64 else []),
             "mag": ["huge-pair-plus", "huge-pair-minus", "huge-opposite", "tiny-pair", "float32-subnormals", "zeros-mixed",
                     "negative-zeros", "constant"]}
    want = sorted(f"{group}/{kind}" for group, kinds in named.items() for kind in kinds)
    assert sorted(set(labels)) == want
    assert want == sorted(mc.kinds_at(K))
    # a single NaN at every row that is a multiple of 64 or of 100
    rows = sorted(int(np.flatnonzero(np.isnan(m[:, j]))[0]) for j in np.flatnonzero(labels == "nan/row-multiple-64-or-100"))
    assert rows == sorted(set(range(64, K, 64)) | set(range(100, K, 100)))
    with np.errstate(all="ignore"):
        constant = np.all(m == m[0], axis=0) | np.all(np.isnan(m), axis=0)
    assert sorted(set(labels[constant])) == sorted(mc.ALL_EQUAL_KINDS)
    for kind in ("random/distinct", "order/ascending", "order/organ-pipe", "order/blocks64-descending"):
        for j in np.flatnonzero(labels == kind):
            assert np.unique(m[:, j]).size == K, (kind, "values are not distinct")
    for j in np.flatnonzero(np.char.startswith(labels, "two/")):
        assert set(m[:, j].tolist()) == {mc.LOW, mc.HIGH}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 17, 100, 101, 256, 300, 1200, 1201])
def test_special_kinds_give_what_they_claim(K, dtype):
    m, labels = _columns(K, dtype)
    ref = mc.reference_median(m)
    has_nan = np.isnan(m).any(axis=0)
    with np.errstate(all="ignore"):
        total = m.astype(np.float64).sum(axis=0)

    def of(kind):
        found = np.flatnonzero(labels == kind)
        assert found.size > 0, kind
        return found

    assert np.array_equal(has_nan, np.char.startswith(labels, "nan/"))
    assert np.all(np.isnan(ref[has_nan])), "a NaN in a column gives NaN"
    assert np.all(ref[of("inf/plus-majority")] == np.inf) and np.all(ref[of("inf/minus-majority")] == -np.inf)
    for kind in ("inf/one-plus", "inf/one-minus", "inf/one-each", "inf/both-in-block64", "inf/both-in-block100"):
        assert np.all(np.isfinite(ref[of(kind)])), kind
    # +inf and -inf in one column: its sum is NaN without any NaN in it (the kernels' detection takes its rare path)
    for kind in ("inf/one-each", "inf/both-in-block64", "inf/both-in-block100"):
        assert np.all(np.isnan(total[of(kind)])) and not has_nan[of(kind)].any(), kind
    if K % 2 == 0:
        assert np.all(ref[of("inf/plus-exactly-half")] == np.inf), "the middle pair is (finite, +inf)"
        assert np.all(np.isnan(ref[of("inf/half-minus-half-plus")])) and not has_nan[of("inf/half-minus-half-plus")].any()
        assert np.all(ref[of("mag/huge-opposite")] == 0.0)
    for kind, L in (("inf/both-in-block64", 64), ("inf/both-in-block100", 100), ("inf/different-block64", 64),
                    ("inf/different-block100", 100), ("nan/two-different-blocks", 64)):
        if kind not in mc.kinds_at(K):
            continue
        for j in of(kind):
            r = np.flatnonzero(~np.isfinite(m[:, j]))
            assert r.size == 2 and (r[0] // L == r[1] // L) == ("both-in" in kind), (kind, r)
    huge = np.float64(np.finfo(np.float32).max) if dtype == "float32" else np.float64(1.7e308)
    overflows = (K % 2 == 0) and dtype == "float64"  # 1.7e308 + 1.7e308; twice float32's largest value is a double
    assert np.all(ref[of("mag/huge-pair-plus")] == (np.inf if overflows else huge))
    assert np.all(ref[of("mag/huge-pair-minus")] == (-np.inf if overflows else -huge))
    tiny = (2.0 ** -149, 2.0 ** -148) if dtype == "float32" else (5e-324, 1e-323)
    (j,) = of("mag/tiny-pair")
    s = np.sort(m[:, j].astype(np.float64))
    assert (s[(K - 1) // 2], s[(K - 1) // 2 + 1]) == tiny
    assert ref[j] == (tiny[0] if K % 2 else (tiny[0] + tiny[1]) / 2.0) and ref[j] > 0.0
    (j,) = of("mag/float32-subnormals")
    col = m[:, j].astype(np.float64)
    assert np.all(np.abs(col) < 2.0 ** -126) and np.all(col != 0.0) and np.all(col.astype(np.float32).astype(np.float64) == col)
    assert ref[j] != 0.0
    (j,) = of("mag/zeros-mixed")
    assert np.all(m[:, j] == 0.0) and ref[j] == 0.0
    assert np.all(np.signbit(m[:, of("mag/negative-zeros")[0]]))


def test_two_valued_builders():
    m = mc.two_valued_exhaustive(5)
    assert m.shape == (5, 32) and len({tuple(c) for c in m.T.tolist()}) == 32 and set(m.ravel().tolist()) == {mc.LOW, mc.HIGH}
    for K in (3, 20, 101):
        m = mc.two_valued_balanced(K, 999, seed=1)
        high = (m == mc.HIGH).sum(axis=0)
        assert m.shape == (K, 999) and np.all((m == mc.HIGH) | (m == mc.LOW))
        assert set(high.tolist()) == set(range(max(0, K // 2 - 2), min(K, K // 2 + 2) + 1))
        assert mc.mismatch(mc.reference_median(m), mc.sorted_median(m), None, K) is None


def test_regimes():
    sweep = [k for name in mc.SWEEP_RANGES for k in mc.ks_for(f"sweep-{name}")]
    assert sweep == list(range(1, 1211))
    assert mc.ks_for("exhaustive")[:15] == list(range(2, 17))
    assert set(mc.ks_for("balanced-networks")) >= {17, 19, 20, 21, 23, 24, 97, 99, 100}
