"""median.hip in every K regime and on adversarial columns (tests/median_cases.py), against np.median as the reference
project calls it: every K from 1 to 1210 (every selection network exact and padded, the two-halves kernel, every parts
configuration with 0 to L - 1 padding entries and with whole padding parts, the rank-counting kernel), every 0-1 column
for the networks up to 20 inputs, balanced 0-1 samples above, the batch kernel with its statistics, and the order
statistic, mean and trimmed mean kernels around the sizes at which NumPy's pairwise sum changes shape."""
import numpy as np
import pytest

import median_cases as mc

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")


def _median(m):
    import torch

    from rocco_amd import rocco as rr

    return rr.score_central_tendency_chrom_device(torch.from_numpy(m).cuda()).cpu().numpy()


def _assert_all(failures):
    assert not failures, f"{len(failures)} failures; first: " + " | ".join(failures[:5])


# ---- a. every K ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ks", mc.SWEEP_RANGES)
def test_every_k(gpu, ks, dtype):
    failures = []
    for K in mc.ks_for(f"sweep-{ks}"):
        m, labels = mc.columns(K, dtype, seed=K)
        message = mc.mismatch(_median(m), mc.reference_median(m), labels, K)
        if message is not None:
            failures.append(message)
    _assert_all(failures)


# ---- b. every 0-1 column: a min / max network that is right on all of them is right on every input -----------------------
@pytest.mark.parametrize("K", mc.ks_for("exhaustive"))
def test_every_two_valued_column(gpu, K):
    m = mc.two_valued_exhaustive(K)
    message = mc.mismatch(_median(m), mc.reference_median(m), None, K)
    assert message is None, message + " (the column's number in binary is its rows, row 0 lowest; 1 = HIGH)"


@pytest.mark.parametrize("K", mc.ks_for("sampled-24"))
def test_sampled_two_valued_columns_of_the_24_network(gpu, K):
    # 2**24 columns of 24 rows are 3 GB and half a minute of NumPy: 2**18 + 5 sampled columns around the balance instead
    m = mc.two_valued_balanced(K, 2 ** 18 + 5, seed=K)
    message = mc.mismatch(_median(m), mc.reference_median(m), None, K)
    assert message is None, message


# ---- c. balanced 0-1 samples ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mc.ks_for("balanced-networks") + mc.ks_for("balanced-large"))
def test_balanced_two_valued_columns(gpu, K):
    m = mc.two_valued_balanced(K, 20007 if K <= 600 else 5003, seed=K)  # (fewer above 600: the host reference's seconds)
    got, want = _median(m), mc.reference_median(m)
    message = mc.mismatch(got, want, None, K)
    if message is not None:
        j = int(np.flatnonzero(got != want)[0])
        message += f"; rows holding HIGH: {np.flatnonzero(m[:, j] == mc.HIGH).tolist()}"
    assert message is None, message


# ---- d. the batch kernel and its statistics -------------------------------------------------------------------------------
def _batch_matrices(K, dtype):
    """Three matrices cut from columns(K) in a shuffled order (n = 1, 64 and the rest) and a fourth of every column without a
    NaN in it: for an even K that one holds a score that is NaN from inf - inf alone."""
    m, labels = mc.columns(K, dtype, seed=1000 + K)
    labels = np.array(labels)
    order = np.random.default_rng(K).permutation(m.shape[1])
    clean = np.flatnonzero(~np.isnan(m).any(axis=0))
    picks = [order[:1], order[1:65], order[65:], clean]
    if K % 2 == 0:
        ref = mc.reference_median(m[:, clean])
        assert np.isnan(ref).any() and "inf/half-minus-half-plus" in labels[clean]
    mats = []
    for p in picks:
        cut = np.empty((K, len(p)), dtype=m.dtype)  # (a fresh array: a one-column slice keeps the stride of its source)
        cut[...] = m[:, p]
        mats.append((cut, labels[p]))
    return mats


def _stats_failure(row, scores):
    """The rule of test_gpu_median_stats.py for [min, max, sum |.|] of a score array, with NaN and infinite scores."""
    keep = ~np.isnan(scores)
    if keep.any() and not (row[0] == scores[keep].min() and row[1] == scores[keep].max()):
        return f"min / max {row[0]!r} / {row[1]!r}, want {scores[keep].min()!r} / {scores[keep].max()!r}"
    with np.errstate(all="ignore"):
        total = np.abs(scores).sum()
    if np.isnan(scores).any():  # from a NaN in the column or from inf - inf in its middle pair alike
        ok = np.isnan(row[2])
    elif np.isinf(total):
        ok = row[2] == np.inf
    else:
        ok = abs(row[2] - total) <= 1e-12 * max(1.0, total)
    return None if ok else f"sum |.| {row[2]!r}, want {total!r}"


def _batch_failures(K, dtype, with_stats):
    import torch

    from rocco_amd import rocco as rr

    mats = _batch_matrices(K, dtype)
    tensors = [torch.from_numpy(m).cuda() for m, _ in mats]
    assert all(t.stride(1) == 1 for t in tensors), "a matrix would be scored by the launch per matrix, not by the batch"
    if with_stats:
        outs, stats = rr.score_central_tendency_chrom_batch_device(tensors, with_stats=True)
        assert stats is not None and tuple(stats.shape) == (len(mats), 3)
        stats = stats.cpu().numpy()
    else:
        outs = rr.score_central_tendency_chrom_batch_device(tensors)
    failures = []
    for i, ((m, labels), out) in enumerate(zip(mats, outs)):
        want = mc.reference_median(m)
        message = mc.mismatch(out.cpu().numpy(), want, labels, K)
        if message is None and with_stats:
            message = _stats_failure(stats[i], want)
            message = None if message is None else f"K={K}: {message}"
        if message is not None:
            failures.append(f"matrix {i} (n={m.shape[1]}) {message}")
    return failures


@pytest.mark.parametrize("with_stats", (False, True), ids=("scores", "stats"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_kernel_every_k(gpu, dtype, with_stats):
    failures = []
    for K in mc.ks_for("batch"):
        failures += _batch_failures(K, dtype, with_stats)
    _assert_all(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", mc.ks_for("batch-fallback"))
def test_batch_fallback_statistics(gpu, K, dtype):
    _assert_all(_batch_failures(K, dtype, True))


# ---- e. order statistic, mean, trimmed mean -------------------------------------------------------------------------------
def _method_columns(K):
    """The finite, tied, +-inf and magnitude kinds of columns(K) and one column with a NaN."""
    m, labels = mc.columns(K, "float64", seed=2000 + K)
    labels = np.array(labels)
    keep = ~np.char.startswith(labels, "nan/")
    keep[np.flatnonzero(labels == "nan/row-0")[0]] = True
    return np.ascontiguousarray(m[:, keep]), labels[keep]


def _method(m, **kwargs):
    import torch

    from rocco_amd import rocco as rr

    return rr.score_central_tendency_chrom_device(torch.from_numpy(m).cuda(), **kwargs).cpu().numpy()


def _bits_failure(got, want, exact, labels, K, what):
    """Equal bit for bit where `exact`, equal with NaNs in the same places elsewhere."""
    message = mc.mismatch(got, want, labels, K)
    if message is None and got[exact].tobytes() != want[exact].tobytes():
        j = int(np.flatnonzero(exact)[np.flatnonzero(got[exact].view(np.int64) != want[exact].view(np.int64))[0]])
        message = f"K={K}: column {j} ({labels[j]}): got {got[j]!r}, want {want[j]!r} (bits differ)"
    return None if message is None else f"{what}: {message}"


@pytest.mark.parametrize("K", mc.ks_for("methods"))
def test_order_statistic(gpu, K):
    m, labels = _method_columns(K)
    ordered = np.sort(m, axis=0)  # NaN last
    has_nan = np.isnan(m).any(axis=0)
    failures = []
    for rank in (range(K) if K <= 17 else sorted({0, 1, K // 3, K // 2, K - 2, K - 1})):
        want = np.where(has_nan, np.nan, ordered[rank])
        message = mc.mismatch(_method(m, method="rank", rank=rank), want, labels, K)
        if message is not None:
            failures.append(f"rank {rank}: {message}")
    _assert_all(failures)


@pytest.mark.parametrize("K", mc.ks_for("methods"))
def test_column_mean(gpu, K):
    m, labels = _method_columns(K)
    with np.errstate(all="ignore"):
        want = np.mean(m, axis=0)
    message = _bits_failure(_method(m, method="mean"), want, np.isfinite(m).all(axis=0), labels, K, "mean")
    assert message is None, message


@pytest.mark.parametrize("K", mc.ks_for("methods"))
def test_trimmed_mean(gpu, K):
    from scipy import stats

    m, labels = _method_columns(K)
    ordered = np.sort(m, axis=0)
    failures = []
    for tprop in (0.0, 0.05, 0.2, 0.5):
        ramp = np.arange(K, dtype=float)  # the ranks as rocco.py computes them
        lo, hi = int(np.quantile(ramp, tprop, method="nearest")), int(np.quantile(ramp, 1.0 - tprop, method="nearest"))
        assert lo <= hi
        with np.errstate(all="ignore"):
            want = np.array([stats.tmean(m[:, i], limits=(ordered[lo, i], ordered[hi, i]), inclusive=(True, True))
                             for i in range(m.shape[1])])
        # (columns whose values tie at a limit: the two-valued ones, and the ties and counts among the random ones)
        message = _bits_failure(_method(m, method="tmean", rank=lo, rank_hi=hi), want, np.isfinite(want), labels, K,
                                f"tprop {tprop} (ranks {lo}, {hi})")
        if message is not None:
            failures.append(message)
    _assert_all(failures)
