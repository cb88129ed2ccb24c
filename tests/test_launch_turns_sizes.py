"""No GPU: the caps the library states (rocco_hip_launch_caps) and the whole size logic of tests/test_gpu_launch_turns.py.  Every
`*_size` function of tests/launch_turns_cases.py asserts that its case reaches a second turn under the caps; a cap changed
in include/rocco_hip.h that would quietly turn a case back into a first-turn case fails here, where there is no device."""
import ctypes

import numpy as np

import launch_turns_cases as lt
from locus_summaries_cases import NumpyVector


def test_the_caps_are_the_headers_and_every_one_is_named():
    from rocco_amd import _native

    caps = _native.launch_caps()
    assert list(caps) == list(_native.LAUNCH_CAP_NAMES) and all(isinstance(v, int) and v > 0 for v in caps.values())
    guarded = (ctypes.c_int * (len(caps) + 1))(*([-7] * (len(caps) + 1)))
    _native.load().rocco_hip_launch_caps(guarded)
    assert list(guarded)[:-1] == list(caps.values()) and guarded[len(caps)] == -7  # ROCCO_LAUNCH_CAPS entries, not one more
    # the getters that were there before keep their lengths and agree where they state the same number
    from rocco_amd import bam, readtracks

    assert bam.bam_shape()["threads"] == caps["bam_threads"]
    shape = readtracks.fragment_length_shape()
    assert (shape["threads"], shape["density_records"], shape["density_window"]) == (
        caps["fragment_threads"], caps["fragment_density_records"], caps["fragment_density_window"])
    for name in caps:
        if name.endswith("_threads"):
            assert caps[name] % 64 == 0, name


def test_every_case_reaches_a_second_turn_under_the_caps():
    c = lt.caps()
    n = lt.select_single_size(c)
    assert n > c["select_grid_target"] * c["select_chunk_values"]
    second = lt.select_second_turn_first_value(n, n, c)
    ((blocks, chunks),) = lt.select_blocks([n], c)
    assert second == blocks * c["select_chunk_values"] < n and blocks < chunks
    lengths = lt.select_group_sizes(c)
    assert sum(lengths) > c["select_grid_target"] * c["select_chunk_values"] and lengths[0] > 2 * lengths[1] > 8 * lengths[2]
    for k, (blocks, chunks) in enumerate(lt.select_blocks(lengths, c)):
        assert lt.select_second_turn_first_value(lengths[k], sum(lengths), c) == blocks * c["select_chunk_values"] < lengths[k]
    assert lt.bh_size(c) > c["bh_max_grid"] * c["bh_threads"]
    assert lt.chrom_range_size(c) > c["chrom_range_max_grid"] * c["count_threads"]
    assert lt.count_tail_size(c) > c["count_tail_max_grid"] * c["count_threads"]
    assert lt.interval_facts_size(c) > c["interval_facts_max_grid"] * c["count_intervals_threads"]
    sizes = lt.flag_facts_sizes(c)
    assert sizes[0] > c["fragment_max_grid"] * c["fragment_threads"] and sizes[1] == 0
    assert lt.template_size(c) > c["fragment_max_grid"] * c["fragment_threads"] + 100
    assert lt.density_size(c) > c["fragment_max_grid"] * c["fragment_density_records"]
    bam = lt.bam_sizes(c)
    assert bam["records"] > bam["first_record_of_second_turn"] == c["bam_max_grid"] * c["bam_threads"]


def test_second_turn_refuses_sizes_that_have_none():
    for items, unit, cap in ((2048 * 256, 256, 2048), (2048 * 256 - 1, 256, 2048), (2 * 2048 * 256 + 1, 256, 2048), (2049 * 256, 256, 2048)):
        try:
            lt.second_turn(items, unit, cap)
        except AssertionError:
            continue
        raise AssertionError((items, unit, cap))
    assert lt.second_turn(2048 * 256 + 1, 256, 2048) == 2048 * 256


def test_the_partition_reference_is_the_sorting_one():
    """`launch_turns_cases.select_expected_bits` (one np.partition, for vectors of 17 M values) against
    `locus_summaries_cases.NumpyVector.select` (a full sort in key order) on a vector with ties, signed zeros, infinities
    and NaNs of either sign, in both modes."""
    x = lt.select_vector(70000, 3, 60000, 70000)
    x[[5, 50000]] = [np.nan, -np.nan]
    ranks = [0, 1, 2, 3, 9999, 10000, 10001, 35000, 59999, 60000, 69990, 69995, 69996, 69997, 69998, 69999]
    for mode, center in ((0, 0.0), (1, 0.37), (1, -1000.0)):
        want = NumpyVector(x).select(ranks, mode, center)
        assert lt.select_expected_bits(x, ranks, mode, center) == [
            0x7FFFFFFFFFFFFFFF if np.isnan(w) else int(np.float64(w).view(np.uint64)) for w in want], (mode, center)
    assert lt.select_expected_bits(x, [0, 69999])[0] == int(np.float64(-np.inf).view(np.uint64))


def test_the_builders_put_the_deciding_fact_in_the_turn_they_say():
    c = lt.caps()
    for second in (True, False):
        fields, _, _, passing = lt.chrom_range_case(c, second)
        turn = c["chrom_range_max_grid"] * c["count_threads"]
        assert passing.size > 100 and ((passing.min() > turn) if second else (passing.max() < turn))
        _, at, _ = lt.interval_long_record_case(c, second)
        assert (at > c["interval_facts_max_grid"] * c["count_intervals_threads"]) == second
    for where in ("second", "first", "both"):
        positive = np.flatnonzero(lt.count_tail_counts(c, where) > 0)
        turn = c["count_tail_max_grid"] * c["count_threads"]
        assert positive.size > 300 and {"second": positive.min() > turn, "first": positive.max() < turn,
                                        "both": positive.min() < turn < positive.max()}[where]
    pos, _, contig_length, _, turn = lt.density_case(c)
    assert np.all(np.diff(pos.astype(np.int64)) >= 0) and contig_length > int(pos[-1])
    assert int(pos[turn + 2000]) - int(pos[turn]) < 250 and int(pos[-1]) - int(pos[turn + 2200]) > 250 * c["fragment_density_window"]
