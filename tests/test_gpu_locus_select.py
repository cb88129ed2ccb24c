"""GPU: rocco_hip_select_ranks_batch_f64 (csrc/select.hip) against np.sort in the select's key order -- every rank of the
short fixture vectors, 16 spread ranks of the long ones, bit for bit; batches of unequal lengths, past the 48 vectors of
one series of launches and with rank lists that differ; mode 1 against |x - c| over the finite values; the four counts."""
import numpy as np
import pytest

from locus_summaries_cases import NumpyVector, golden

pytestmark = pytest.mark.gpu


def _select(gpu, vectors, ranks, mode=0, centers=None):
    import torch

    from rocco_amd.inference import select_ranks_batch_device

    tensors = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(gpu) for v in vectors]
    values, counts = select_ranks_batch_device(tensors, ranks, mode, centers)
    return values.cpu().numpy(), counts.cpu().numpy()


def _score_vectors():
    return {key[len("scores_"):]: value for key, value in golden().items() if key.startswith("scores_")}


def _spread(n, k=16):
    return sorted({int(r) for r in np.linspace(0, n - 1, k)} | {0, n - 1})[:k] if n > k else list(range(n))


def _check(values, counts, vector, ranks, mode=0, center=0.0):
    want = NumpyVector(vector).select(ranks, mode, center)
    assert np.asarray(values, dtype=np.float64).view(np.uint64).tolist() == \
        [(0x7FFFFFFFFFFFFFFF if np.isnan(w) else int(np.float64(w).view(np.uint64))) for w in want]
    assert tuple(int(c) for c in counts) == NumpyVector(vector).counts()


def test_every_rank_of_the_short_vectors_and_spread_ranks_of_the_long_ones(gpu):
    for name, vector in _score_vectors().items():
        n = vector.shape[0]
        if n <= 300:
            for first in range(0, n, 16):
                ranks = list(range(first, min(first + 16, n)))
                ranks += [ranks[-1]] * (0 if first == 0 else 16 - len(ranks))  # (a full list: duplicates are allowed)
                values, counts = _select(gpu, [vector], [ranks])
                _check(values[0], counts[0], vector, ranks)
        else:
            ranks = _spread(n)
            values, counts = _select(gpu, [vector], [ranks[::-1]])  # (any order)
            _check(values[0], counts[0], vector, ranks[::-1])


def test_signed_zeros_sort_by_key(gpu):
    vector = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, np.nan, -np.nan, np.inf, -np.inf])
    ranks = list(range(10))
    values, counts = _select(gpu, [vector], [ranks])
    assert np.signbit(values[0][:5]).tolist() == [True, True, True, True, False] and values[0][2] == 0.0 and values[0][4] == 0.0
    _check(values[0], counts[0], vector, ranks)
    assert counts[0].tolist() == [2, 1, 1, 6]


def test_batch_of_unequal_lengths_with_rank_lists_that_differ(gpu):
    vectors = _score_vectors()
    batch = [vectors["gamma49157"], vectors["gamma1"], vectors["mixed"], vectors["nan"], vectors["inf"]]
    ranks = [[49156, 0, 24578, 16384], [0, 0, 0, 0], [999, 500, 1, 0], [256, 0, 255, 128], [3, 2, 253, 254]]
    values, counts = _select(gpu, batch, ranks)
    for v in range(len(batch)):
        _check(values[v], counts[v], batch[v], ranks[v])
    assert np.isnan(values[3][0]) and values[3][2] == np.sort(batch[3])[255]  # the one NaN sorts last
    finite = batch[4][np.isfinite(batch[4])]
    assert values[4][0] == finite.min() and np.isneginf(values[4][1]) and values[4][2] == finite.max() and np.isposinf(values[4][3])


def test_fifty_vectors_are_served_past_the_forty_eight_of_one_series(gpu):
    gen = np.random.default_rng(48)
    batch = [np.round(gen.normal(0.0, 2.0, size=int(gen.integers(1, 400))), 1) + 0.0 for _ in range(50)]
    ranks = [[0, (v.shape[0] - 1) // 2, v.shape[0] // 2, v.shape[0] - 1, int(gen.integers(0, v.shape[0]))] for v in batch]
    values, counts = _select(gpu, batch, ranks)
    for v in range(50):
        _check(values[v], counts[v], batch[v], ranks[v])


def test_counts_alone_need_no_rank_and_take_an_empty_vector(gpu):
    vectors = _score_vectors()
    batch = [vectors["inf"], np.zeros(0), vectors["nan"], vectors["negative"], vectors["zeros90"]]
    values, counts = _select(gpu, batch, [[] for _ in batch])
    assert values.shape == (5, 0)
    for v in range(5):
        assert tuple(int(c) for c in counts[v]) == NumpyVector(batch[v]).counts()


def test_mode_one_selects_among_absolute_deviations_of_the_finite_values(gpu):
    vectors = _score_vectors()
    batch = [vectors["inf"], vectors["nan"], vectors["mixed"], vectors["gamma49157"], vectors["last_digit"]]
    centers = [1.37, 2.5, -0.3, 3.01, 1.0 + 150 * 2.0 ** -52]
    ranks = [_spread(v.shape[0], 12) for v in batch]
    ranks = [r + [r[-1]] * (12 - len(r)) for r in ranks]
    values, counts = _select(gpu, batch, ranks, 1, centers)
    for v in range(len(batch)):
        _check(values[v], counts[v], batch[v], ranks[v], 1, centers[v])
        finite = batch[v][np.isfinite(batch[v])]
        want = np.sort(np.abs(finite - centers[v]))
        for r, got in zip(ranks[v], values[v]):
            assert (np.isnan(got) and r >= finite.shape[0]) or got.tobytes() == want[r].tobytes()


def test_mostly_zeros_and_all_equal_over_three_chunks(gpu):
    vectors = _score_vectors()
    for name in ("zeros90", "equal"):
        vector = vectors[name]
        ranks = _spread(vector.shape[0])
        values, counts = _select(gpu, [vector], [ranks])
        _check(values[0], counts[0], vector, ranks)
    long_zeros = np.zeros(3 * 16384 + 5)
    long_zeros[::10] = np.round(np.random.default_rng(90).gamma(2.0, 1.5, size=long_zeros[::10].shape[0]), 2)
    ranks = _spread(long_zeros.shape[0])
    values, counts = _select(gpu, [long_zeros], [ranks])
    _check(values[0], counts[0], long_zeros, ranks)


def test_invalid_arguments_are_refused(gpu):
    vector = np.arange(5.0)
    with pytest.raises(ValueError):
        _select(gpu, [vector], [[5]])  # a rank past the end
    with pytest.raises(ValueError):
        _select(gpu, [np.zeros(0)], [[0]])  # a rank of an empty vector
    with pytest.raises(ValueError):
        _select(gpu, [vector], [list(range(5)) * 4])  # more than 16 ranks in one call
