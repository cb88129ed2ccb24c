"""GPU: scoring views.  `score_central_tendency_chrom_device` and its batch form pass a matrix's `stride(0)` to the kernels
as the row stride, and the driver hands a caller's CUDA tensors to them as they are (rocco_amd/rocco.py:550-558, 626):
a column slice `big[:, a:a + n]` of a wider tensor has row stride > n and an element offset that may be odd.  Every
median regime (selection network, two halves, parts, rank kernel), the order statistic, the mean and the trimmed mean on
such views must give what they give on `.contiguous()` and what NumPy / SciPy give on the host copy, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 777  # three full 256-locus workgroups and a partial one


def _view(gpu, K, n, a, dtype, seed, pad=45):
    """A [K, n] column slice starting at column `a` of a [K, a + n + pad] device tensor whose other columns are NaN (a
    kernel that reads outside the view shows)."""
    import torch

    rng = np.random.default_rng(seed)
    host = np.round(rng.gamma(1.0, 0.3, size=(K, n)), 2).astype(dtype)  # plenty of ties
    big = torch.full((K, a + n + pad), float("nan"), dtype=getattr(torch, np.dtype(dtype).name), device=gpu)
    view = big[:, a:a + n]
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) == a + n + pad > n and view.storage_offset() == a
    return host, view


@pytest.mark.parametrize("K", [2, 7, 100, 101, 150, 200, 256, 601, 1201])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_median_of_a_view(gpu, K, dtype):
    from rocco_amd import rocco as rr

    host, view = _view(gpu, K, N, 13, dtype, seed=K)
    got = rr.score_central_tendency_chrom_device(view).cpu().numpy()
    assert np.array_equal(got, rr.score_central_tendency_chrom_device(view.contiguous()).cpu().numpy())
    assert np.array_equal(got, np.median(host.astype(np.float64), axis=0)), K


@pytest.mark.parametrize("K", [2, 7, 100, 101, 256, 1201])
def test_order_statistic_mean_and_trimmed_mean_of_a_view(gpu, K):
    from scipy import stats

    from rocco_amd import rocco as rr

    host, view = _view(gpu, K, N, 7, "float64", seed=500 + K)
    ordered = np.sort(host, axis=0)
    for rank in sorted({0, K // 3, K - 1}):
        got = rr.score_central_tendency_chrom_device(view, method="rank", rank=rank).cpu().numpy()
        assert np.array_equal(got, rr.score_central_tendency_chrom_device(view.contiguous(), method="rank", rank=rank).cpu().numpy())
        assert np.array_equal(got, ordered[rank]), (K, rank)
    got = rr.score_central_tendency_chrom_device(view, method="mean").cpu().numpy()
    assert got.tobytes() == rr.score_central_tendency_chrom_device(view.contiguous(), method="mean").cpu().numpy().tobytes()
    assert got.tobytes() == np.mean(host, axis=0).tobytes(), K
    ramp = np.arange(K, dtype=float)
    lo, hi = int(np.quantile(ramp, 0.05, method="nearest")), int(np.quantile(ramp, 0.95, method="nearest"))
    got = rr.score_central_tendency_chrom_device(view, method="tmean", rank=lo, rank_hi=hi).cpu().numpy()
    same = rr.score_central_tendency_chrom_device(view.contiguous(), method="tmean", rank=lo, rank_hi=hi).cpu().numpy()
    assert got.tobytes() == same.tobytes()
    want = np.array([stats.tmean(host[:, i], limits=(ordered[lo, i], ordered[hi, i]), inclusive=(True, True)) for i in range(N)])
    assert got.tobytes() == want.tobytes(), K


@pytest.mark.parametrize("K", [7, 100, 150])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_median_batch_of_views(gpu, K, dtype):
    """60 views of ONE device tensor (past one launch of 48), of 1, 255, 256, 257 and a few thousand loci, each at an odd
    element offset: the batch with and without the statistics against the batch of contiguous copies and NumPy."""
    import torch

    from rocco_amd import rocco as rr

    rng = np.random.default_rng(K)
    ns = [(1, 255, 256, 257, 3001, 2, 64)[i % 7] for i in range(60)]
    host = np.round(rng.gamma(1.0, 0.4, size=(K, sum(ns) + 2 * len(ns) + 1)), 3).astype(dtype) - 0.2
    big = torch.from_numpy(host).to(gpu)
    views, hosts, at = [], [], 1
    for n in ns:
        views.append(big[:, at:at + n])
        hosts.append(host[:, at:at + n])
        at += n + (1 if n % 2 else 2)
    assert all(v.stride(0) > v.shape[1] and v.storage_offset() % 2 == 1 for v in views)
    medians = [np.median(h.astype(np.float64), axis=0) for h in hosts]
    copies = [v.contiguous() for v in views]
    plain = rr.score_central_tendency_chrom_batch_device(views)
    plain_c = rr.score_central_tendency_chrom_batch_device(copies)
    for i, (o, c, s) in enumerate(zip(plain, plain_c, medians)):
        assert np.array_equal(o.cpu().numpy(), c.cpu().numpy()) and np.array_equal(o.cpu().numpy(), s), i
    outs, st = rr.score_central_tendency_chrom_batch_device(views, with_stats=True)
    outs_c, st_c = rr.score_central_tendency_chrom_batch_device(copies, with_stats=True)
    assert st is not None and st_c is not None
    st, st_c = st.cpu().numpy(), st_c.cpu().numpy()
    for i, (o, s) in enumerate(zip(outs, medians)):
        assert np.array_equal(o.cpu().numpy(), s), i
        assert st[i][0] == s.min() and st[i][1] == s.max() and st_c[i][0] == st[i][0] and st_c[i][1] == st[i][1], i
        assert abs(st[i][2] - np.abs(s).sum()) <= 1e-12 * max(1.0, np.abs(s).sum()), i
