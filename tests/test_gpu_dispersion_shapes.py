"""GPU: score_dispersion_chrom on every template shape of rocco_amd/csrc/dispersion.hip -- each of the eleven network sizes
in its exact form (K == KP) and at the lowest and the highest K of its padded form -- on SIGNED data with adversarial
columns (zeros of both signs, sorted orders, outliers, infinities walked across MAD's balanced padding, finite entries whose
sums overflow, subnormals, cancellation); column counts at the workgroup and XCD boundaries; and long columns, where the
pairwise order needs its fourth written-out level.  Expected values are NumPy's and SciPy's alone, every comparison is exact
(the standard of `same` in tests/test_gpu_dispersion.py: equal values, NaN where NaN is wanted, the sign of a zero).

The ONE relaxation: iqr on a column that holds both -0.0 and +0.0.  The two compare equal, so which of them np.partition
leaves at a percentile's position is an accident of its algorithm, and with it the sign of a zero answer: NumPy itself defines
the value only, and those columns (`dispersion_expected.both_zeros`) are compared with np.array_equal."""
import numpy as np
import pytest
from scipy import stats

import dispersion_expected as de
from test_gpu_dispersion import quiet

pytestmark = pytest.mark.gpu

SHAPE_TPROPS = {"f64": (0.0, 0.05, 0.2, 0.5), "f32": (0.2,)}
BOUNDARY_KS = (16, 81)  # a network size no other dispersion test reaches, and the shape that reads the column twice
BOUNDARY_NS = (1, 2, 255, 256, 257, 1792, 2048, 2049, 4097)  # 1, 1, 1, 1, 2, 7, 8, 9 and 17 workgroups
PERIOD = 257  # coprime to the 256 columns of a workgroup: a misplaced workgroup meets other columns
LONG_TPROPS = (0.0, 0.05)


@pytest.fixture(scope="module")
def trimmed_want():
    """The per-column SciPy loops of every test of this module, computed once in worker processes (no torch, no GPU there)."""
    jobs = [("signed", K, de.SHAPE_N, dtype, tprop, True) for K in de.SHAPE_KS for dtype in ("f64", "f32") for tprop in SHAPE_TPROPS[dtype]]
    jobs += [("signed", K, de.SHAPE_N, dtype, 0.05, False) for K in de.SHAPE_KS for dtype in ("f64", "f32")]
    jobs += [("signed", K, PERIOD, "f64", 0.05, False) for K in BOUNDARY_KS]
    jobs += [("long", K, de.LONG_N, "f64", tprop, True) for K in de.LONG_KS for tprop in LONG_TPROPS]
    jobs += [("long", K, de.LONG_N, "f64", 0.05, False) for K in de.LONG_KS]
    return dict(zip(jobs, de.trimmed_expected(jobs)))


def differing(got, want, names, values_only=None):
    """The columns where `got` is not `want`: [(column, name, got, want)], at most eight.  `values_only`: columns whose zero
    answers may carry either sign (see the head of this file)."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    sign = (np.signbit(got) != np.signbit(want)) & ~np.isnan(want)
    if values_only is not None:
        sign &= ~values_only
    where = np.flatnonzero(bad | sign)
    return [(int(j), names[j % len(names)], float(got[j]), float(want[j])) for j in where[:8]]


def test_the_k_list_reaches_every_template_shape():
    shapes = {(de.network_size(K), K == de.network_size(K)) for K in de.SHAPE_KS}
    # (the padded form of KP = 2 is instantiated but has no K: K = 1 is answered before any kernel)
    assert shapes == {(kp, exact) for kp in de.NETWORK_SIZES for exact in (True, False)} - {(2, False)} and len(shapes) == 21
    # both ends of every padded range: KP - K decides MAD's padding, the tail of the pairwise sums and the second read
    lowest = {kp: min(K for K in de.SHAPE_KS if de.network_size(K) == kp) for kp in de.NETWORK_SIZES}
    assert [lowest[kp] for kp in de.NETWORK_SIZES] == [2] + [kp + 1 for kp in de.NETWORK_SIZES[:-1]]
    assert all(kp - 1 in de.SHAPE_KS for kp in de.NETWORK_SIZES[1:])


@pytest.mark.parametrize("dtype", ("f64", "f32"))
@pytest.mark.parametrize("K", de.SHAPE_KS)
def test_every_network_shape_on_signed_and_adversarial_columns(gpu, trimmed_want, K, dtype):
    import torch

    from rocco_amd import score_dispersion_chrom
    from rocco_amd.rocco import score_dispersion_chrom_device

    m, names = de.signed_matrix(K, de.SHAPE_N, dtype)
    wide = np.asarray(m, dtype=float)
    mixed = de.both_zeros(wide)
    assert names.count("plain") > 400 and mixed[names.index("-0.0 +0.0 in turn")] and not mixed[names.index("all -0.0")]
    wrong = {}
    wrong["mad"] = differing(score_dispersion_chrom(m, method="mad"), quiet(stats.median_abs_deviation, wide, axis=0), names)
    wrong["std"] = differing(score_dispersion_chrom(m, method="std"), quiet(np.std, wide, axis=0), names)
    for rng in de.SHAPE_RNGS:
        # values only on the columns that hold both zeros, the sign as well everywhere else
        wrong[f"iqr {rng}"] = differing(score_dispersion_chrom(m, method="iqr", rng=rng), quiet(stats.iqr, wide, rng=rng, axis=0), names,
                                        values_only=mixed)
    for tprop in SHAPE_TPROPS[dtype]:
        got = score_dispersion_chrom(m, method="tstd", tprop=tprop)
        wrong[f"tstd {tprop}"] = differing(got, trimmed_want[("signed", K, de.SHAPE_N, dtype, tprop, True)], names)
    got = score_dispersion_chrom_device(torch.from_numpy(m).to(gpu), method="tstd", root=False).cpu().numpy()
    wrong["tvar"] = differing(got, trimmed_want[("signed", K, de.SHAPE_N, dtype, 0.05, False)], names)
    assert {check: columns for check, columns in wrong.items() if columns} == {}


@pytest.mark.parametrize("K", (6, 10, 14, 22, 30, 46, 62, 78, 90))
def test_even_k_in_the_padded_forms(gpu, K):
    """The padded K of the list above are all odd (the ends of the ranges are).  An even K takes the mean of two middle
    values, in MAD beside the -inf / +inf padding: with 1.5e308 throughout that mean overflows and the median is +inf
    though every entry is finite -- SciPy answers +inf, and NaN only where an entry is +inf itself.  The exact forms
    answered NaN for both before they counted the entries equal to the median; the padded forms are held to the same."""
    from rocco_amd import score_dispersion_chrom

    m, names = de.signed_matrix(K, 130, "f64")
    assert K < de.network_size(K) and {"huge throughout", "huge throughout and one +inf", "huge throughout and one -inf"} <= set(names)
    want = quiet(stats.median_abs_deviation, m, axis=0)
    assert np.isposinf(want[names.index("huge throughout")]) and np.isposinf(want[names.index("huge throughout and one -inf")])
    assert np.isnan(want[names.index("huge throughout and one +inf")])
    wrong = {"mad": differing(score_dispersion_chrom(m, method="mad"), want, names),
             "std": differing(score_dispersion_chrom(m, method="std"), quiet(np.std, m, axis=0), names),
             "iqr": differing(score_dispersion_chrom(m, method="iqr"), quiet(stats.iqr, m, axis=0), names, values_only=de.both_zeros(m))}
    assert {check: columns for check, columns in wrong.items() if columns} == {}


@pytest.mark.parametrize("K", BOUNDARY_KS)
def test_column_counts_at_the_workgroup_and_xcd_boundaries(gpu, trimmed_want, K):
    """Every column count is the 257-column matrix tiled along the columns and cut at n, so the expected vector is the
    tiled expected vector.  The device form writes into a view of a longer tensor whose guard must stay as it was."""
    import torch

    from rocco_amd.rocco import score_dispersion_chrom_device

    base, names = de.signed_matrix(K, PERIOD, "f64")
    tvar = trimmed_want[("signed", K, PERIOD, "f64", 0.05, False)]
    want = {"mad": quiet(stats.median_abs_deviation, base, axis=0), "iqr": quiet(stats.iqr, base, axis=0), "std": quiet(np.std, base, axis=0),
            "tstd": quiet(np.sqrt, tvar)}  # the device form takes the correctly rounded root of SciPy's variance
    mixed, guard = de.both_zeros(base), 64
    wrong = {}
    for n in BOUNDARY_NS:
        reps = -(-n // PERIOD)
        m_t = torch.from_numpy(np.ascontiguousarray(np.tile(base, (1, reps))[:, :n])).to(gpu)
        for method in ("mad", "iqr", "std", "tstd"):
            expected = np.tile(want[method], reps)[:n]
            if method == "std" and n == 1:
                expected = np.std(base[:, :1].copy(), axis=0)  # the K x 1 matrix: NumPy's pairwise order
            out_t = torch.full((n + guard,), -7.0, dtype=torch.float64, device=gpu)
            back = score_dispersion_chrom_device(m_t, out_t=out_t[:n], method=method)
            assert back.data_ptr() == out_t.data_ptr() and back.shape == (n,)
            host = out_t.cpu().numpy()
            assert np.array_equal(host[n:], np.full(guard, -7.0)), (n, method)
            wrong[(n, method)] = differing(host[:n], expected, names, values_only=np.tile(mixed, reps)[:n] if method == "iqr" else None)
    # K x 1 matrices that are no constant: an adversarial column and a plain one in NumPy's pairwise order
    for j in (names.index("ascending"), names.index("ascending") + 1, names.index("subnormal")):
        column = np.ascontiguousarray(base[:, j:j + 1])
        got = score_dispersion_chrom_device(torch.from_numpy(column).to(gpu), method="std").cpu().numpy()
        wrong[("single column", j)] = differing(got, quiet(np.std, column, axis=0), names[j:j + 1])
    assert {check: columns for check, columns in wrong.items() if columns} == {}


@pytest.mark.parametrize("K", de.LONG_KS)
def test_long_columns_on_the_memory_path(gpu, trimmed_want, K):
    """K > 100: rank counting and the written-out pairwise order.  K = 969 and K = 1023 leave a block of more than 128 terms
    after three levels of NumPy's uneven split (969 -> 480 + 489 -> ... -> 129): with the order written out to three levels
    both failed here in tstd, in the variance and in the single-column std.  The last column alternates +-1.5e308: finite
    entries, and NaN from NumPy's pairwise sums (one accumulator +inf, its neighbour -inf)."""
    import torch

    from rocco_amd import score_dispersion_chrom
    from rocco_amd.rocco import score_dispersion_chrom_device

    m, names = de.long_matrix(K)
    assert m.shape == (K, de.LONG_N) and names[64] == "+-huge in turn"
    wrong = {}
    wrong["mad"] = differing(score_dispersion_chrom(m, method="mad"), quiet(stats.median_abs_deviation, m, axis=0), names)
    wrong["std"] = differing(score_dispersion_chrom(m, method="std"), quiet(np.std, m, axis=0), names)
    mixed = de.both_zeros(m)
    for rng in ((25, 75), (0, 100)):
        wrong[f"iqr {rng}"] = differing(score_dispersion_chrom(m, method="iqr", rng=rng), quiet(stats.iqr, m, rng=rng, axis=0), names,
                                        values_only=mixed)
    for tprop in LONG_TPROPS:
        want = trimmed_want[("long", K, de.LONG_N, "f64", tprop, True)]
        assert np.isnan(want[64]) and np.isfinite(want[2:64]).all()
        wrong[f"tstd {tprop}"] = differing(score_dispersion_chrom(m, method="tstd", tprop=tprop), want, names)
    got = score_dispersion_chrom_device(torch.from_numpy(m).to(gpu), method="tstd", root=False).cpu().numpy()
    wrong["tvar"] = differing(got, trimmed_want[("long", K, de.LONG_N, "f64", 0.05, False)], names)
    # np.std of a K x 1 matrix: the pairwise order, on eight fresh columns and on the overflowing one
    singles = [2.0 * np.random.default_rng([K, seed]).standard_normal((K, 1)) for seed in range(8)] + [np.ascontiguousarray(m[:, 64:65])]
    for i, column in enumerate(singles):
        want = quiet(np.std, column.copy(), axis=0)
        assert bool(np.isnan(want[0])) == (i == 8)
        got = score_dispersion_chrom_device(torch.from_numpy(column).to(gpu), method="std").cpu().numpy()
        wrong[("single column", i)] = differing(got, want, ["K x 1"])
    assert {check: columns for check, columns in wrong.items() if columns} == {}


def test_one_row_past_the_pairwise_limit_still_raises(gpu):
    import torch

    from rocco_amd.rocco import score_dispersion_chrom_device

    tall = torch.from_numpy(de.signed_matrix(1025, 3, "f64", adversarial=False)[0]).to(gpu)
    with pytest.raises(ValueError, match="at most 1024 rows"):
        score_dispersion_chrom_device(tall, method="tstd")
    with pytest.raises(ValueError, match="at most 1024 rows"):
        score_dispersion_chrom_device(tall[:, 2:3], method="std")
