"""Row f6 without a GPU: the NumPy statement of the interval counts against every count the reference's compiled counter
wrote (tests/golden/interval_count_vectors.*), the three host ports of rocco/scores.py against the reference's recorded
outputs and error texts, the argument checks of the new entry points, and the premise of the 2**24 clamp."""
import os

import numpy as np
import pytest

import interval_counts_expected as iv


@pytest.fixture(scope="module")
def gold():
    return iv.load_golden()


def test_statement_equals_every_fixture_count(gold):
    arrays, meta = gold
    checked = 0
    for option_name, options in meta["options"].items():
        for key in meta["files"]:
            for contig in meta["contigs"]:
                want = arrays[f"c_{option_name}_{key}_{contig}"]
                assert want.dtype == np.float32
                got = iv.count_intervals(iv.fields_of(arrays, key, contig), arrays[f"iv_{contig}_start"], arrays[f"iv_{contig}_end"],
                                         **options)
                assert np.array_equal(got.astype(np.float32), want), (option_name, key, contig)
                checked += want.size
    assert checked >= 5 * 3 * 3 * 200


def test_fixture_covers_what_the_issue_names(gold):
    arrays, meta = gold
    pile = meta["pile_position"]
    starts, ends = arrays["iv_chrA_start"], arrays["iv_chrA_end"]
    size = meta["contigs"]["chrA"]
    assert (ends - starts).min() == 1 and (ends - starts).max() >= size
    assert np.any(ends > size) and np.any(ends <= arrays["f_s1_chrA_pos"].min()) and np.any(starts > arrays["f_s1_chrA_pos"].max())
    assert np.any((starts < pile) & (ends > pile)) and np.any(starts == pile)
    pairs = set(zip(starts.tolist(), ends.tolist()))
    assert len(pairs) < starts.size  # repeated intervals
    assert np.any(np.diff(starts) < 0)  # not sorted
    assert int(np.sum(arrays["f_s1_chrA_pos"] == pile)) >= 3000
    assert arrays["c_raw_count_matrix_s1_chrA"].max() >= 3000
    assert all(meta["files"][key]["chrE"] == 0 for key in meta["files"])


def test_random_intervals_port(gold, tmp_path):
    from rocco_amd import scores

    _, meta = gold
    sizes = tmp_path / "g.sizes"
    sizes.write_text(meta["sizes_text"])
    for case in meta["random_intervals"]:
        got = scores._random_intervals(str(sizes), length=case["length"], nsamples=case["nsamples"], seed=case["seed"])
        assert [list(t) for t in got] == case["intervals"], case
        assert all(type(t[0]) is str and type(t[1]) is int and type(t[2]) is int for t in got)
    with pytest.raises(ValueError) as info:
        scores._random_intervals(str(sizes), length=meta["random_intervals_error"]["length"], nsamples=5, seed=1)
    assert str(info.value) == meta["random_intervals_error"]["message"].replace("{file}", str(sizes))


def test_assign_length_bins_port(gold):
    from rocco_amd import scores

    arrays, meta = gold
    for case in meta["assign_length_bins"]:
        binned, reps = scores._assign_length_bins(arrays[f"alb_{case['name']}_lengths"], max_bins=case["max_bins"],
                                                  min_bin_width_bp=case["min_bin_width_bp"])
        for got, want in ((binned, arrays[f"alb_{case['name']}_binned"]), (reps, arrays[f"alb_{case['name']}_reps"])):
            assert got.dtype == want.dtype and np.array_equal(got, want), case
    with pytest.raises(ValueError) as info:
        scores._assign_length_bins(np.zeros(0))
    assert str(info.value) == meta["assign_length_bins_error"]


def test_read_peak_intervals_port(gold, tmp_path):
    from rocco_amd import scores

    _, meta = gold
    peaks = tmp_path / "peaks.bed"
    peaks.write_text(meta["peaks_text"])
    chroms, starts, ends, bed_strings, names = scores._read_peak_intervals(str(peaks), min_columns=3)
    want = meta["read_peak_intervals"]
    assert (chroms, starts, ends, bed_strings, names) == (want["chroms"], want["starts"], want["ends"], want["bed_strings"], want["names"])
    short = tmp_path / "short.bed"
    short.write_text(meta["read_peak_intervals_error"]["text"])
    with pytest.raises(ValueError) as info:
        scores._read_peak_intervals(str(short), min_columns=3)
    assert str(info.value) == meta["read_peak_intervals_error"]["message"]
    with pytest.raises(ValueError) as info:
        scores._read_peak_intervals(str(peaks), min_columns=5)
    assert str(info.value) == meta["read_peak_intervals_error5"]["message"]


def records(n=4):
    from rocco_amd.readtracks import AlignmentRecords

    pos = np.arange(n, dtype=np.int32) * 10
    return AlignmentRecords(pos, pos + 5, np.zeros(n, np.int32), np.zeros(n, np.uint16), np.full(n, 30, np.uint8), np.ones(n, np.uint8))


def test_interval_arguments_are_checked_before_any_device_work():
    from rocco_amd.readtracks import count_alignment_intervals_batch_device, count_alignment_intervals_from_records

    one = [{"chrA": records()}]
    with pytest.raises(ValueError, match="each interval must satisfy end > start"):
        count_alignment_intervals_batch_device(one, ["chrA", "chrA"], [0, 7], [5, 7])
    with pytest.raises(ValueError, match="each interval must satisfy end > start"):
        count_alignment_intervals_from_records(one[0], ["chrA"], [9], [3])
    with pytest.raises(ValueError, match="must have the same length"):
        count_alignment_intervals_batch_device(one, ["chrA", "chrA"], [0], [5, 7])
    with pytest.raises(ValueError, match="must have the same length"):
        count_alignment_intervals_batch_device(one, ["chrA"], [0, 1], [5, 7])
    with pytest.raises(ValueError, match=r"\[0, 2\*\*31\)"):
        count_alignment_intervals_batch_device(one, ["chrA"], [-1], [5])
    with pytest.raises(ValueError, match=r"\[0, 2\*\*31\)"):
        count_alignment_intervals_batch_device(one, ["chrA"], [0], [2**31])
    with pytest.raises(ValueError, match="chromosome not found in alignment header"):
        count_alignment_intervals_batch_device(one, ["chrA", "chrQ"], [0, 0], [5, 5])
    with pytest.raises(ValueError, match="chromosome not found in alignment header"):
        count_alignment_intervals_batch_device([{"chrA": records()}, {"chrB": records()}], ["chrA"], [0], [5])
    with pytest.raises(ValueError, match="count mode `cutsite` is not built"):
        count_alignment_intervals_batch_device(one, ["chrA"], [0], [5], count_mode="cutsite")
    with pytest.raises(ValueError, match="no files"):
        count_alignment_intervals_batch_device([], ["chrA"], [0], [5])
    with pytest.raises(TypeError):
        count_alignment_intervals_batch_device(one, ["chrA"], [0.5], [5])


def test_composed_arguments_are_checked(gold, tmp_path):
    from rocco_amd import scores

    _, meta = gold
    peaks, sizes, empty = tmp_path / "peaks.bed", tmp_path / "g.sizes", tmp_path / "empty.bed"
    peaks.write_text(meta["peaks_text"])
    sizes.write_text(meta["sizes_text"])
    empty.write_text("\n")
    one = [{"chrA": records()}]
    with pytest.raises(ValueError, match="one sample name per file"):
        scores.raw_count_matrix_from_records(one, ["a", "b"], str(peaks), str(tmp_path / "out.tsv"))
    with pytest.raises(ValueError, match="Peak file does not contain any intervals."):
        scores.raw_count_matrix_from_records(one, ["a"], str(empty), str(tmp_path / "out.tsv"))
    with pytest.raises(ValueError, match="`sample_scaling_constants` must match the number of BAM files."):
        scores.get_ecdf_from_records(one, 100, str(sizes), nsamples=3, sample_scaling_constants=[1.0, 2.0], seed=1)
    with pytest.raises(ValueError, match="`files_per_call` must be at least 1"):
        scores._interval_counts_device(one, ["chrA"], [0], [5], 0)
    with pytest.raises(ValueError, match="one sample name, mapped count and read length per file"):
        scores.score_peaks_from_records(one, ["a"], str(sizes), str(peaks), [1, 2], [50])


def test_float32_stops_counting_at_two_to_the_24():
    """The reference adds 1.0f into one float per interval: the premise of the clamp in the float32 mirror."""
    assert np.float32(2**24) + np.float32(1) == np.float32(2**24)
    assert np.float32(2**24 - 1) + np.float32(1) == np.float32(2**24)
    total = np.float32(2**24 - 2)
    for _ in range(5):
        total = np.float32(total + np.float32(1.0))
    assert total == np.float32(2**24)


def test_count_matrix_reader_keeps_integers_integer(tmp_path):
    from rocco_amd import scores

    path = tmp_path / "m.tsv"
    path.write_text("peak_name\ta\tb\nchr_1_2\t3\t4\nchr_5_9\t0\t17\n")
    got = scores._read_count_matrix(str(path))
    assert got.dtype == np.int64 and got.tolist() == [[3, 4], [0, 17]]
    got[:, 0] = got[:, 0] * 2.9  # what score_peaks does next: truncation toward zero inside the integer array
    assert got[:, 0].tolist() == [8, 0]
    path.write_text("peak_name\ta\nchr_1_2\t3.5\n")
    assert scores._read_count_matrix(str(path)).dtype == np.float64
