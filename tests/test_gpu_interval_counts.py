"""Row f6 on the GPU: decoded alignment records -> one count per (interval, file) (rocco_amd/csrc/interval_count.hip)
against every count the reference's compiled counter wrote (tests/golden/interval_count_vectors.*), bit for bit, and
against the NumPy statement of the same arithmetic (tests/interval_counts_expected.py, pinned to those fixtures by
tests/test_interval_counts_host.py) at the sizes where the kernels change path.

A pair (interval, file) has `unit` candidate records per work unit; a wavefront takes one unit at a time and the counting
launch has `grid` workgroups of `waves` wavefronts at most (further units are taken in a grid stride); the library
reports the three numbers (rocco_hip_count_intervals_shape)."""
import numpy as np
import pytest

import alignment_counts_expected as expected
import interval_counts_expected as iv

pytestmark = pytest.mark.gpu
RAW = dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10)


@pytest.fixture(scope="module")
def gold():
    return iv.load_golden()


@pytest.fixture(scope="module")
def shape(gpu):
    from rocco_amd.readtracks import count_intervals_shape

    s = count_intervals_shape()
    assert s["unit_records"] > 0 and s["unit_records"] % 64 == 0 and s["max_grid"] > 0 and s["waves_per_group"] > 0
    return s


def to_records(fields):
    from rocco_amd.readtracks import AlignmentRecords

    return AlignmentRecords(*fields)


@pytest.fixture(scope="module")
def gold_records(gold):
    arrays, meta = gold
    return {key: {contig: to_records(iv.fields_of(arrays, key, contig)) for contig in meta["contigs"]} for key in meta["files"]}


def all_intervals(arrays, meta):
    contigs, starts, ends = [], [], []
    for contig in meta["contigs"]:
        s, e = arrays[f"iv_{contig}_start"], arrays[f"iv_{contig}_end"]
        contigs += [contig] * s.size
        starts.append(s)
        ends.append(e)
    order = np.random.default_rng(3).permutation(len(contigs))  # contigs interleaved
    return np.asarray(contigs)[order], np.concatenate(starts)[order], np.concatenate(ends)[order], order


def wanted(arrays, meta, option_name, key, order):
    return np.concatenate([arrays[f"c_{option_name}_{key}_{contig}"] for contig in meta["contigs"]])[order]


def test_every_fixture_count_in_one_call_per_option_set(gpu, gold, gold_records):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    arrays, meta = gold
    contigs, starts, ends, order = all_intervals(arrays, meta)
    files = list(meta["files"])
    for option_name, options in meta["options"].items():
        got = count_alignment_intervals_batch_device([gold_records[key] for key in files], contigs, starts, ends, **options)
        assert got.dtype.is_floating_point is False and tuple(got.shape) == (len(contigs), len(files)) and got.is_cuda
        got = got.cpu().numpy()
        assert got.dtype == np.int32
        for f, key in enumerate(files):
            want = wanted(arrays, meta, option_name, key, order)
            assert np.array_equal(got[:, f].astype(np.float32), want) and np.array_equal(got[:, f], want.astype(np.int32)), (option_name, key)


def test_every_fixture_count_through_the_float32_mirror(gpu, gold, gold_records):
    from rocco_amd.readtracks import count_alignment_intervals_from_records

    arrays, meta = gold
    contigs, starts, ends, order = all_intervals(arrays, meta)
    for option_name, options in meta["options"].items():
        for key in meta["files"]:
            got = count_alignment_intervals_from_records(gold_records[key], list(contigs), list(starts), list(ends), thread_count=3,
                                                         infer_fragment_length=0, count_mode="coverage", **options)
            want = wanted(arrays, meta, option_name, key, order)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want.tobytes(), (option_name, key)


def test_three_files_in_one_call_equal_three_calls(gpu, gold, gold_records):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    arrays, meta = gold
    contigs, starts, ends, _ = all_intervals(arrays, meta)
    files = list(meta["files"])
    options = meta["options"]["paired"]
    together = count_alignment_intervals_batch_device([gold_records[key] for key in files], contigs, starts, ends, **options).cpu().numpy()
    for f, key in enumerate(files):
        alone = count_alignment_intervals_batch_device([gold_records[key]], contigs, starts, ends, **options).cpu().numpy()
        assert alone.shape == (len(contigs), 1) and np.array_equal(alone[:, 0], together[:, f]), key


@pytest.fixture(scope="module")
def uniform_track():
    """4 000 records of one span (50) on distinct ascending positions 100, 110, ...: the candidates of an interval are the
    records with start - 50 < pos < end, so their number is chosen exactly."""
    n = 4000
    rng = np.random.default_rng(12)
    pos = (100 + 10 * np.arange(n)).astype(np.int32)
    flag = np.where(rng.random(n) < 0.5, 0, 16).astype(np.uint16)
    flag |= np.where(rng.random(n) < 0.1, 4, 0).astype(np.uint16)
    return (pos, (pos + 50).astype(np.int32), np.zeros(n, np.int32), flag, rng.integers(0, 61, size=n).astype(np.uint8),
            np.ones(n, np.uint8))


def test_candidate_counts_around_the_unit(gpu, shape, uniform_track):
    """Pairs with 0, 1, UNIT - 1, UNIT, UNIT + 1 and 3 UNIT + 5 candidates (and neighbours), in one call and one by one."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    unit = shape["unit_records"]
    pos = uniform_track[0].astype(np.int64)
    starts, ends, candidates = [], [], []
    for k in (0, 1, 2, unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 1, 3 * unit + 5):
        for first in (0, 7, 1500):
            # candidates: pos in (start - 50, end) = the k records first .. first + k - 1 (fewer than six only at the
            # head of the track: the window is at least 50 positions wide and the records lie 10 apart)
            if k == 0:
                start, end = 5, 51
            elif k < 6:
                start, end = 60, int(pos[k - 1]) + 1
            else:
                start, end = int(pos[first]) + 41, int(pos[first + k - 1]) + 1
            starts.append(start)
            ends.append(end)
            candidates.append(int(np.sum((pos > start - 50) & (pos < end))))
    assert sorted(set(candidates)) == sorted({0, 1, 2, unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 1, 3 * unit + 5})
    records = {"c": to_records(uniform_track)}
    for options in (RAW, dict(one_read_per_bin=0, flag_exclude=4), dict(one_read_per_bin=1, extend_bp=30, shift_forward_strand53=20)):
        want = iv.count_intervals(uniform_track, starts, ends, **options)
        got = count_alignment_intervals_batch_device([records], ["c"] * len(starts), starts, ends, **options).cpu().numpy()[:, 0]
        assert np.array_equal(got, want), options
        for i in (0, 3, 9, 12, 15, len(starts) - 1):  # P = 1
            single = count_alignment_intervals_batch_device([records], ["c"], [starts[i]], [ends[i]], **options).cpu().numpy()
            assert single.shape == (1, 1) and int(single[0, 0]) == int(want[i]), (options, i)


@pytest.fixture(scope="module")
def deep_track():
    return expected.random_records(np.random.default_rng(5), 40000, 300000)


def test_whole_contig_interval_many_units(gpu, shape, deep_track):
    """One interval over 40 000 records: many units of one pair, the atomic path; run twice: identical."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    assert 40000 > 8 * shape["unit_records"]
    records = {"c": to_records(deep_track)}
    starts, ends = [0, 0, 150000, 299000], [400000, 150000, 400000, 299001]
    for options in (RAW, dict(one_read_per_bin=1, paired_end_mode=1, read_length=50), dict(one_read_per_bin=0, extend_bp=150)):
        want = iv.count_intervals(deep_track, starts, ends, **options)
        assert want[0] > 8 * shape["unit_records"] or options.get("paired_end_mode")
        got = count_alignment_intervals_batch_device([records], ["c"] * 4, starts, ends, **options).cpu().numpy()
        again = count_alignment_intervals_batch_device([records], ["c"] * 4, starts, ends, **options).cpu().numpy()
        assert np.array_equal(got[:, 0], want), options
        assert got.tobytes() == again.tobytes()


def test_more_units_than_the_grid_holds(gpu, shape, deep_track):
    """More units than grid x wavefronts per workgroup in one call: every wavefront takes several units in turn."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    P = shape["max_grid"] * shape["waves_per_group"] + 777
    rng = np.random.default_rng(8)
    starts = rng.integers(0, 299000, size=P)
    ends = starts + rng.integers(1, 900, size=P)
    want = iv.count_intervals(deep_track, starts, ends, **RAW)
    assert np.count_nonzero(want) > shape["max_grid"] * shape["waves_per_group"]
    got = count_alignment_intervals_batch_device([{"c": to_records(deep_track)}], ["c"] * P, starts, ends, **RAW).cpu().numpy()
    assert np.array_equal(got[:, 0], want)


def test_every_interval_empty(gpu, deep_track):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    starts = np.arange(310000, 310000 + 500 * 7, 7)
    got = count_alignment_intervals_batch_device([{"c": to_records(deep_track)}], ["c"] * starts.size, starts, starts + 5, **RAW)
    assert tuple(got.shape) == (starts.size, 1) and int(got.abs().sum()) == 0


def test_empty_tracks_beside_full_ones(gpu, deep_track):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    rng = np.random.default_rng(21)
    other = expected.random_records(rng, 3000, 90000)
    none = tuple(np.zeros(0, dtype=a.dtype) for a in deep_track)
    files = [{"a": deep_track, "b": none, "c": other}, {"a": none, "b": none, "c": none}, {"a": none, "b": other, "c": deep_track}]
    contigs = rng.choice(["a", "b", "c"], size=400)
    starts = rng.integers(0, 299000, size=400)
    ends = starts + rng.integers(1, 5000, size=400)
    want = iv.count_matrix(files, contigs, starts, ends, **RAW)
    got = count_alignment_intervals_batch_device([{k: to_records(v) for k, v in by.items()} for by in files], contigs, starts, ends,
                                                 **RAW).cpu().numpy()
    assert np.array_equal(got, want) and np.all(got[:, 1] == 0) and want[:, 0].max() > 0 and want[:, 2].max() > 0


def test_one_long_record_ahead_of_short_ones(gpu):
    """A 1 Mb record (a spliced read) widens the candidate window of its whole track: more records are read and filtered,
    the counts stay those of the statement."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    rng = np.random.default_rng(31)
    fields = list(expected.random_records(rng, 6000, 1500000, first=1000))
    fields[0][0], fields[1][0], fields[3][0], fields[4][0] = 1000, 1001000, 0, 60
    fields = tuple(fields)
    starts = np.concatenate([rng.integers(0, 1500000, size=300), [0, 999, 1000, 1000999, 1001000, 500000]])
    ends = starts + np.concatenate([rng.integers(1, 3000, size=300), [1, 1, 1, 1, 1, 2]])
    want = iv.count_intervals(fields, starts, ends, **RAW)
    assert want[-3] >= 1 and want[-1] >= 1  # the long record alone reaches there
    got = count_alignment_intervals_batch_device([{"c": to_records(fields)}], ["c"] * starts.size, starts, ends, **RAW).cpu().numpy()
    assert np.array_equal(got[:, 0], want)


def test_unsorted_track_is_refused(gpu, deep_track):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    shuffled = [a.copy() for a in deep_track]
    shuffled[0][[20000, 20001]] = shuffled[0][[20001, 20000]] + np.array([5, -5], dtype=np.int32)
    assert shuffled[0][20000] > shuffled[0][20001]
    files = [{"a": to_records(deep_track), "b": to_records(deep_track)}, {"a": to_records(deep_track), "b": to_records(tuple(shuffled))}]
    with pytest.raises(ValueError, match="file 1 on b are not in coordinate order"):
        count_alignment_intervals_batch_device(files, ["a", "b"], [0, 10], [100, 500], **RAW)
    got = count_alignment_intervals_batch_device(files[:1], ["a", "b"], [0, 10], [100, 500], **RAW)  # the sorted file alone passes
    assert tuple(got.shape) == (2, 1)
