"""Host side of score_dispersion_chrom (no GPU): the helpers that turn `rng` / `tprop` / K into the kernel arguments
against NumPy's own functions, the errors that need no device, the fixture against this host's NumPy / SciPy, and the
arithmetic the kernels are written to -- restated in NumPy scalars -- against np.std and stats.tstd."""
import json
import os
import warnings

import numpy as np
import pytest
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
RNGS = ((25, 75), (10, 90), (12.5, 87.5), (0, 100), (33, 66.6), (75, 25), (50, 50), (1, 99))
KS = tuple(range(2, 41)) + (50, 63, 64, 65, 99, 100, 101, 127, 128, 129, 137, 200, 255, 256, 257, 300)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "dispersion_vectors.npz"))


def test_the_function_is_exported_under_the_reference_name():
    import rocco_amd
    from rocco_amd import score_dispersion_chrom  # noqa: F401  (rocco/__init__.py star-exports it from rocco/rocco.py)
    from rocco_amd.rocco import score_dispersion_chrom_device  # noqa: F401

    assert rocco_amd.score_dispersion_chrom is score_dispersion_chrom


def lerp(a, b, g):
    """The rule of include/rocco_hip.h (rocco_hip_score_percentile_range), in float64 scalars."""
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


@pytest.mark.parametrize("K", KS)
def test_percentile_taps_reproduce_np_percentile_on_sorted_columns(K):
    from rocco_amd.rocco import _percentile_range_taps, _percentile_tap

    gen = np.random.default_rng(K)
    for column in (np.arange(K, dtype=float), np.sort(np.round(gen.gamma(2.0, 1.5, K), 2)), np.sort(gen.normal(size=K))):
        for q in (0, 1, 10, 12.5, 25, 33, 50, 66.6, 75, 87.5, 90, 99, 100, 0.1, 99.9, 37.123):
            index, g = _percentile_tap(K, q)
            assert 0 <= index <= K - 1 and 0.0 <= g < 1.0
            got = lerp(column[index], column[min(index + 1, K - 1)], g)
            assert np.float64(got).tobytes() == np.float64(np.percentile(column, q)).tobytes(), (K, q)
        for rng in RNGS:
            i0, g0, i1, g1 = _percentile_range_taps(K, rng)
            got = lerp(column[i1], column[min(i1 + 1, K - 1)], g1) - lerp(column[i0], column[min(i0 + 1, K - 1)], g0)
            assert np.float64(got).tobytes() == np.float64(stats.iqr(column, rng=rng)).tobytes(), (K, rng)


@pytest.mark.parametrize("K", KS)
def test_trim_ranks_pick_what_np_quantile_nearest_picks(K):
    from rocco_amd.rocco import _trim_ranks

    column = np.sort(np.random.default_rng(1000 + K).normal(size=K))  # distinct values: the rank is identified
    for tprop in (0.0, 0.01, 0.05, 0.1, 0.2, 0.25, 1.0 / 3.0, 0.45, 0.5):
        lo, hi = _trim_ranks(K, tprop)
        assert column[lo] == np.quantile(column, tprop, method="nearest")
        assert column[hi] == np.quantile(column, 1.0 - tprop, method="nearest")


def test_range_validation_is_scipys():
    from rocco_amd.rocco import _percentile_range_taps

    for bad in ((25, 101), (-1, 75), (100.0001, 3)):
        with pytest.raises(ValueError, match=r"^Percentiles must be in the range \[0, 100\]$"):
            _percentile_range_taps(9, bad)
        with pytest.raises(ValueError, match=r"^Percentiles must be in the range \[0, 100\]$"):
            stats.iqr(np.arange(9.0), rng=bad)
    with pytest.raises(TypeError, match="^quantile range must be two element sequence$"):
        _percentile_range_taps(9, (25, 50, 75))
    with pytest.raises(ValueError, match="^range must not contain NaNs$"):
        _percentile_range_taps(9, (25, float("nan")))
    assert _percentile_range_taps(9, (75, 25)) == _percentile_range_taps(9, (25, 75))


def test_errors_that_need_no_device_are_the_recorded_ones(golden):
    from rocco_amd import score_dispersion_chrom

    seen = set()
    for text in golden["errors"]:
        entry = json.loads(str(text))
        if entry["kwargs"].get("method") == "tstd":
            continue  # the reference's own failure, recorded as the stated divergence
        matrix = golden[f"matrix_{entry['matrix']}"] if "matrix" in entry else np.zeros(entry["shape"])
        with pytest.raises(ValueError) as info:
            score_dispersion_chrom(matrix, **entry["kwargs"])
        assert type(info.value).__name__ == entry["class"] and str(info.value) == entry["text"]
        seen.add(entry["text"])
    assert len(seen) == 3
    # K = 1 returns before the method is looked at, on the host
    for power in (1.0, 2, 0):
        got = score_dispersion_chrom(np.ones((1, 7)), method="no such method", power=power)
        assert got.dtype == np.float64 and np.array_equal(got, np.power(np.zeros(7), power))


def test_the_fixture_is_what_this_hosts_numpy_and_scipy_compute(golden):
    counted = 0
    for i, text in enumerate(golden["cases"]):
        case = json.loads(str(text))
        m = np.asarray(golden[f"matrix_{case['matrix']}"], dtype=float)
        method = case["method"].strip().lower().replace("-", "").replace("_", "")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if m.shape[0] == 1:
                want = np.zeros(m.shape[1])
            elif method == "mad":
                want = stats.median_abs_deviation(m, axis=0)
            elif method == "iqr":
                want = stats.iqr(m, rng=case.get("rng", (25, 75)), axis=0)
            else:
                assert method == "std"
                want = np.std(m, axis=0)
            want = np.power(want, case.get("power", 1.0))
        assert want.dtype == np.float64 and np.array_equal(want, golden[f"expected_{i}"], equal_nan=True), case
        counted += 1
    assert counted == len(golden["cases"]) >= 150


# ---- the arithmetic of the kernels, restated ------------------------------------------------------------------------

def pairwise_sum(a):
    """NumPy's pairwise order over a 1-D float64 array (what pairwise() of dispersion.hip unrolls)."""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for x in a:
            res = res + x
        return res
    if n <= 128:
        r = [np.float64(x) for x in a[:8]]
        i = 8
        while i < n - n % 8:
            for q in range(8):
                r[q] = r[q] + a[i + q]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in a[i:]:
            res = res + x
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def tvar_restated(c, lo, hi):
    """The trimmed variance as include/rocco_hip.h (rocco_hip_score_trimmed_std, take_root == 0) states it."""
    keep = ~((c < lo) | (c > hi))
    cnt = np.float64(keep.sum())
    mean = pairwise_sum(np.where(keep, c, 0.0)) / cnt
    d = c - mean
    var = pairwise_sum(np.where(keep, d * d, 0.0)) / cnt
    if cnt <= 1.0:
        return np.float64(np.nan)
    return var * (cnt / (cnt - 1.0))


@pytest.mark.parametrize("K", (2, 3, 5, 7, 8, 9, 10, 15, 16, 17, 33, 64, 100, 101, 128, 129, 137, 255, 256, 257, 300, 968, 969, 1023, 1024))
def test_restated_trimmed_variance_and_root_are_scipys_per_column(K):
    """Pins the SPECIFICATION, not a kernel: the arithmetic dispersion.hip's tstd is written after (dropped values as
    0.0, NumPy's pairwise order, kept / (kept - 1), the scalar `** 0.5`) is what this host's SciPy computes.  Of the
    project's code only `_trim_ranks` takes part; the kernels are held to SciPy in tests/test_gpu_dispersion.py."""
    from rocco_amd.rocco import _trim_ranks

    gen = np.random.default_rng(77 + K)
    m = np.round(gen.gamma(2.0, 1.5, size=(K, 40)), 2)
    m[:, 0] = 1.25
    for tprop in (0.0, 0.05, 0.2, 0.5):
        rank_lo, rank_hi = _trim_ranks(K, tprop)
        lo = np.quantile(m, tprop, axis=0, method="nearest")
        hi = np.quantile(m, 1.0 - tprop, axis=0, method="nearest")
        for j in range(m.shape[1]):
            column = np.sort(m[:, j])
            assert column[rank_lo] == lo[j] and column[rank_hi] == hi[j]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = stats.tvar(m[:, j], limits=(lo[j], hi[j]), inclusive=(True, True))
                want_root = stats.tstd(m[:, j], limits=(lo[j], hi[j]), inclusive=(True, True))
            got = tvar_restated(m[:, j], lo[j], hi[j])
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (K, tprop, j)
            # SciPy's root is `** 0.5` on a NumPy scalar (libm's pow), which score_dispersion_chrom repeats on the host
            assert np.float64(got ** 0.5).tobytes() == np.float64(want_root).tobytes(), (K, tprop, j)


@pytest.mark.parametrize("K", (2, 3, 7, 8, 9, 33, 100, 101, 128, 129, 137, 256, 257, 300, 968, 969, 1023, 1024))
def test_restated_std_orders_are_numpys(K):
    """Pins the SPECIFICATION, not a kernel, and touches no project code: the two summation orders dispersion.hip's std
    is written after (row after row for n > 1, pairwise for the single column) are this host's NumPy's.  If a NumPy
    release changes either order this fails first and says why the GPU tests then do."""
    gen = np.random.default_rng(5 + K)
    m = np.round(gen.gamma(2.0, 1.5, size=(K, 30)), 2)
    # n > 1: the rows one after the other
    acc = m[0].copy()
    for k in range(1, K):
        acc = acc + m[k]
    mean = acc / K
    d = m[0] - mean
    acc = d * d
    for k in range(1, K):
        d = m[k] - mean
        acc = acc + d * d
    assert np.sqrt(acc / K).tobytes() == np.std(m, axis=0).tobytes()
    # n == 1: the single column in the pairwise order
    for j in range(5):
        c = m[:, j]
        mean = pairwise_sum(c) / K
        d = c - mean
        got = np.sqrt(pairwise_sum(d * d) / K)
        assert np.float64(got).tobytes() == np.std(m[:, j:j + 1].copy(), axis=0).tobytes(), (K, j)


# ---- the summation order the kernels compile, on the host, for every length ---------------------------------------------

@pytest.fixture(scope="module")
def pairwise_order_check(tmp_path_factory):
    """tests/tools/pairwise_order_check.cpp: rocco_amd/csrc/pairwise_sum.h -- the functions dispersion.hip compiles -- in one
    stand-alone host program, without FMA contraction as the kernels are built."""
    import subprocess

    program = str(tmp_path_factory.mktemp("pairwise") / "pairwise_order_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(HERE, "tools", "pairwise_order_check.cpp"),
                    "-o", program], check=True, capture_output=True)
    return program


def pairwise_data(kind):
    gen = np.random.default_rng(1024)
    if kind == "normal":
        return gen.standard_normal(1024)
    if kind == "thirty binades":
        return gen.standard_normal(1024) * np.exp2(gen.integers(-15, 16, size=1024).astype(float))
    assert kind == "overflowing"  # +-1.5e308 in turn: from n = 16 on one accumulator reaches +inf and its neighbour -inf
    return np.where(np.arange(1024) % 2 == 0, 1.5e308, -1.5e308)


@pytest.mark.parametrize("kind", ("normal", "thirty binades", "overflowing"))
def test_the_written_out_pairwise_order_is_np_sum_for_every_length(pairwise_order_check, tmp_path, kind):
    """Every n in 1 ... 1024 (the K that tstd and the single-column std take) at the depth the kernels use: the bit pattern
    of the sum against np.sum of the contiguous prefix; a NaN (the third data set: inf - inf between two accumulators) must
    be a NaN.  The halves of NumPy's split are uneven, so a depth that serves n = 1024 need not serve every n below it:
    written out to three levels the order is another for every n in 969 ... 1023 that is no multiple of 8 (a block of 129 to 135
    terms is left unsplit), and the sums of each data set differ in the last place at some of those n and nowhere else."""
    import subprocess

    data = np.ascontiguousarray(pairwise_data(kind), dtype=np.float64)
    path = tmp_path / "values.f64"
    path.write_bytes(data.tobytes())
    run = subprocess.run([pairwise_order_check, str(path)], check=True, capture_output=True, text=True, timeout=60)
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == 1024
    wrong, nans = [], 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # overflow and inf - inf inside np.sum
        for n, line in enumerate(lines, start=1):
            n_text, bits = line.split()
            assert int(n_text) == n
            got = np.frombuffer(int(bits, 16).to_bytes(8, "little"), dtype="<f8")[0]
            want = np.sum(data[:n].copy())
            nans += bool(np.isnan(want))
            if not (np.float64(got).tobytes() == np.float64(want).tobytes() or (np.isnan(got) and np.isnan(want))):
                wrong.append(n)
    assert wrong == []
    # the third data set: NumPy's own answer is NaN from n = 16 on (two full rounds of the eight accumulators)
    assert nans == (1024 - 15 if kind == "overflowing" else 0)


# ---- the built kernels use no scratch memory --------------------------------------------------------------------------

def gfx950_code_objects(library):
    """The gfx950 code objects inside the offload bundles of a HIP shared library."""
    import struct

    blob = open(library, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = blob.find(magic)
    while pos >= 0:
        (count,) = struct.unpack_from("<Q", blob, pos + len(magic))
        at = pos + len(magic) + 8
        for _ in range(count):
            offset, size, triple_size = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + triple_size].decode()
            at += 24 + triple_size
            if "gfx950" in triple and size:
                yield blob[pos + offset:pos + offset + size]
        pos = blob.find(magic, pos + 1)


def test_the_dispersion_kernels_have_no_private_segment(tmp_path):
    """Arrays indexed at run time, spilled registers and recursive device functions all end up in scratch memory: every
    kernel of dispersion.hip must report a private segment of 0 bytes in the built library's metadata."""
    import re
    import shutil
    import subprocess

    from rocco_amd import _native

    readelf = shutil.which("llvm-readelf") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    sizes = {}
    for i, code in enumerate(gfx950_code_objects(_native.LIB_PATH)):
        path = tmp_path / f"code{i}.elf"
        path.write_bytes(code)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for kernel in notes.split(".agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", kernel).group(1)
            if re.search(r"dispersion_kernel|dispersion_rank_kernel|std_loop_kernel", name):
                sizes[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", kernel).group(1))
    # 11 network sizes x exact / padded x 4 methods x 2 element types, 3 rank-counting kernels x 2, 2 loop kernels x 2
    assert len(sizes) == 11 * 2 * 4 * 2 + 3 * 2 + 2 * 2
    assert {name: size for name, size in sizes.items() if size != 0} == {}
