"""GPU: the record kernels of rows f5-f8 and the batched select past one launch's first turn.

Every kernel here caps its grid (include/rocco_hip.h: "the grid caps of the record and select kernels"); with more input
than cap x unit a workgroup takes several units in turn.  Real input is always there (a chromosome of a 30x BAM, chr1 at
50 bp, the 62 M scores the composed driver hands the select); the other tests of these kernels never are.  Sizes come from
rocco_hip_launch_caps through tests/launch_turns_cases.py, which asserts for each that some workgroups take two units and
the others one, and builds the input so that what decides the answer lies only where a later turn reads (a mirror case:
only where the first does).  Everything is compared exactly with the host statements the small tests use."""
import numpy as np
import pytest

import alignment_counts_expected as counts_expected
import bam_expected as bx
import fragment_length_expected as fragment_expected
import interval_counts_expected as iv
import launch_turns_cases as lt
from locus_summaries_cases import NumpyVector

pytestmark = pytest.mark.gpu
RAW = dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10)
SEVEN = fragment_expected.FIELDS


@pytest.fixture(scope="module")
def caps(gpu):
    return lt.caps()


def to_records(fields, qlen=None):
    from rocco_amd.readtracks import AlignmentRecords

    return AlignmentRecords(*fields, qlen=qlen)


# ---- the select --------------------------------------------------------------------------------------------------------
def _select(gpu, vectors, ranks, mode=0, centers=None):
    import torch

    from rocco_amd.inference import select_ranks_batch_device

    tensors = [torch.from_numpy(v).to(gpu) for v in vectors]
    values, counts = select_ranks_batch_device(tensors, ranks, mode, centers)
    return values.cpu().numpy(), counts.cpu().numpy()


_single = {}


def single_vector(caps):
    """The single vector, built once for the two tests that read it: its lowest values lie in the chunks a workgroup takes
    in its second turn."""
    if not _single:
        n = lt.select_single_size(caps)
        second = lt.select_second_turn_first_value(n, n, caps)
        assert caps["select_chunk_values"] < n - second < n // 8  # the second turn: more than a chunk, a small part of the vector
        _single.update(n=n, second=second, x=lt.select_vector(n, 7, second, n))
    return _single["n"], _single["second"], _single["x"]


def test_select_single_vector_whose_lowest_values_lie_in_the_second_turn(gpu, caps):
    n, second, x = single_vector(caps)
    ranks = lt.spread_ranks(n, n - second)
    assert len(ranks) == 16 and x[second:].max() < -900 < x[:second][np.isfinite(x[:second])].min()
    values, counts = _select(gpu, [x], [ranks])
    assert values[0].view(np.uint64).tolist() == lt.select_expected_bits(x, ranks)
    assert tuple(int(v) for v in counts[0]) == NumpyVector(x).counts()


def test_select_mode_one_on_the_single_vector(gpu, caps):
    """|x - c| over the finite values: the values of the second turn are the farthest from c, they hold the highest ranks."""
    n, second, x = single_vector(caps)
    center = 0.37
    finite = int(np.isfinite(x).sum())
    far = n - second
    ranks = sorted({int(r) for r in np.linspace(0, finite - far - 1, 11)}) + [finite - far, finite - far // 2, finite - 1, finite, n - 1]
    assert len(ranks) == 16
    values, counts = _select(gpu, [x], [ranks], 1, [center])
    want = lt.select_expected_bits(x, ranks, 1, center)
    assert values[0].view(np.uint64).tolist() == want
    deviations = np.abs(x[np.isfinite(x)] - center)
    assert [int(np.float64(v).view(np.uint64)) for v in np.partition(deviations, ranks[:14])[ranks[:14]]] == want[:14]
    assert want[14] == want[15] == 0x7FFFFFFFFFFFFFFF  # the non-finite values, last, as NaN
    assert tuple(int(v) for v in counts[0]) == NumpyVector(x).counts()


def test_select_group_of_three_strided_vectors_in_either_order(gpu, caps):
    """Three vectors share more than target x chunk values: each is dealt fewer workgroups than it has chunks.  The lowest
    values of each lie in its last chunks (a second turn in either order of the group); rank lists differ per vector."""
    lengths = lt.select_group_sizes(caps)
    total = sum(lengths)
    vectors, ranks, want, low_from = [], [], [], []
    for k, n in enumerate(lengths):
        low_from.append(max(lt.select_second_turn_first_value(n, total, caps), n - 3 * caps["select_chunk_values"] // 2))
        assert low_from[k] < n
        vectors.append(lt.select_vector(n, 20 + k, low_from[k], n))
        ranks.append(lt.spread_ranks(n, n - low_from[k], 16 - k)[: 13] + [k, n - 1 - k, n // (k + 2)])
        assert len(ranks[k]) == 16
        want.append(lt.select_expected_bits(vectors[k], ranks[k]))
    wanted_counts = [NumpyVector(v).counts() for v in vectors]
    for order in ([0, 1, 2], [2, 1, 0]):
        for (blocks, chunks), k in zip(lt.select_blocks([lengths[k] for k in order], caps), order):
            assert blocks < chunks and blocks * caps["select_chunk_values"] <= low_from[k]  # the lowest values: read in a second turn
        values, counts = _select(gpu, [vectors[k] for k in order], [ranks[k] for k in order])
        for at, k in enumerate(order):
            assert values[at].view(np.uint64).tolist() == want[k], (order, k)
            assert tuple(int(v) for v in counts[at]) == wanted_counts[k], (order, k)


# ---- Benjamini-Hochberg ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["second_turn", "first_turn"])
def test_bh_last_passing_rank_beyond_and_inside_the_first_turn(gpu, caps, where):
    import torch

    from rocco_amd.inference import _DeviceVector, benjamini_hochberg_device

    m, fdr, n_nan = lt.bh_size(caps), 0.05, 5
    turn = caps["bh_max_grid"] * caps["bh_threads"]
    passing = [3, 1000, turn - 7] + ([turn + 1, turn + 640] if where == "second_turn" else [])
    p = lt.bh_pvalues(m, passing, n_nan, fdr, 5)
    want_index, want_cutoff = NumpyVector(p).last_passing(fdr)
    assert want_index == n_nan + passing[-1]  # (an index into the device-sorted copy, which the sign-set NaNs lead)
    assert (want_index > turn + n_nan) == (where == "second_turn")
    t = torch.from_numpy(p).to(gpu)
    assert _DeviceVector(t).last_passing(fdr) == (want_index, want_cutoff)
    mask = benjamini_hochberg_device(t, fdr).cpu().numpy()
    assert np.array_equal(mask, lt.bh_mask_numpy(p, fdr)) and np.array_equal(mask, p <= want_cutoff)
    assert int(mask.sum()) == passing[-1] + 1


# ---- chrom range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_second_turn", [True, False])
def test_chrom_range_whose_passing_records_lie_in_one_turn(gpu, caps, in_second_turn):
    from rocco_amd.readtracks import alignment_chrom_range_from_records

    fields, chrom_size, flag_exclude, passing = lt.chrom_range_case(caps, in_second_turn)
    turn = caps["chrom_range_max_grid"] * caps["count_threads"]
    assert (passing.min() > turn) if in_second_turn else (passing.max() < turn)
    want = counts_expected.chrom_range(fields[0], fields[1], fields[3], chrom_size, flag_exclude)
    assert want == (int(fields[0][passing[0]]), int(fields[1][passing[-1]])) and want[1] < int(fields[1][passing].max())
    assert alignment_chrom_range_from_records(to_records(fields), chrom_size, flag_exclude) == want


# ---- count tail --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["second", "first", "both"])
def test_count_tail_whose_positive_bins_lie_in_one_turn_or_in_both(gpu, caps, where):
    import torch

    from rocco_amd import readtracks as rt

    counts = lt.count_tail_counts(caps, where)
    turn = caps["count_tail_max_grid"] * caps["count_threads"]
    positive = np.flatnonzero(counts > 0)
    assert {"second": positive.min() > turn, "first": positive.max() < turn, "both": positive.min() < turn < positive.max()}[where]
    for kw in (dict(norm_scale=0.731, scale_by_step=False, const_scale=1.0, round_digits=5),
               dict(norm_scale=1.9, scale_by_step=True, const_scale=0.37, round_digits=2)):
        want_i, want_v = counts_expected.tail(counts, 4500, 50, **kw)
        got_i, got_v = rt._bam_tail(torch.from_numpy(counts).to(gpu), 4500, 50, kw["norm_scale"], kw["scale_by_step"], kw["const_scale"],
                                    kw["round_digits"], "{file}", "c")
        assert got_i.dtype == want_i.dtype and got_v.dtype == np.float64
        assert got_i.tobytes() == want_i.tobytes() and got_v.tobytes() == want_v.tobytes()


def test_bam_chrom_reads_over_more_bins_and_records_than_a_turn(gpu, caps):
    """The whole path behind get_bam_chrom_reads at a size where the range kernel and the tail kernel are both in their second
    turn: the last tail-reaching record and the last positive bins lie there."""
    from rocco_amd import readtracks as rt

    n = lt.chrom_range_size(caps) + 70000
    step = 10
    bins = lt.count_tail_size(caps)
    fields = counts_expected.random_records(np.random.default_rng(55), n, bins * step - 300, first=100)
    chrom_size = 100 + bins * step
    metadata = dict(read_length=50, resolved_extend_bp=0, paired_end_mode=False, norm_scale=0.013)
    want_i, want_v = counts_expected.bam_chrom_reads(*fields, chrom_size, step, metadata)
    assert want_i.size > caps["count_tail_max_grid"] * caps["count_threads"] and want_v[-1] > 0
    got_i, got_v = rt.bam_chrom_reads_from_records(to_records(fields), chrom_size, step, metadata)
    assert got_i.tobytes() == want_i.tobytes() and got_v.tobytes() == want_v.tobytes()


# ---- interval facts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_second_turn", [True, False])
def test_interval_only_the_one_long_record_reaches(gpu, caps, in_second_turn):
    """The candidate window of every interval is as wide as the track's longest record: the one long record, read by one
    turn only, must widen it."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    fields, at, (start, end) = lt.interval_long_record_case(caps, in_second_turn)
    turn = caps["interval_facts_max_grid"] * caps["count_intervals_threads"]
    assert (at > turn) == in_second_turn
    rng = np.random.default_rng(63)
    starts = np.concatenate([[start, int(fields[0][at]) + 4999], rng.integers(0, int(fields[0][-1]), size=40)])
    ends = np.concatenate([[end, int(fields[0][at]) + 5000], starts[2:] + rng.integers(1, 3000, size=40)])
    want = iv.count_intervals(fields, starts, ends, **RAW)
    assert want[:2].tolist() == [1, 1] and np.count_nonzero(want) > 30
    got = count_alignment_intervals_batch_device([{"c": to_records(fields)}], ["c"] * starts.size, starts, ends, **RAW).cpu().numpy()
    assert np.array_equal(got[:, 0], want)


def test_descent_in_the_second_turn_is_refused_as_an_unsorted_track(gpu, caps):
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    fields, at = lt.interval_descent_case(caps)
    assert at > caps["interval_facts_max_grid"] * caps["count_intervals_threads"]
    good = lt.plain_records(len(fields[0]), 64)
    files = [{"a": to_records(fields)}, {"a": to_records(good)}]
    with pytest.raises(ValueError, match="file 0 on a are not in coordinate order"):
        count_alignment_intervals_batch_device(files, ["a", "a"], [0, 10], [100, 500], **RAW)
    with pytest.raises(ValueError, match="file 1 on a are not in coordinate order"):
        count_alignment_intervals_batch_device(files[::-1], ["a", "a"], [0, 10], [100, 500], **RAW)
    got = count_alignment_intervals_batch_device(files[1:], ["a", "a"], [0, 10], [100, 500], **RAW)  # the sorted file alone passes
    assert tuple(got.shape) == (2, 1)


# ---- flag facts, mapped count ------------------------------------------------------------------------------------------
def test_flag_facts_of_three_tracks_whose_boundary_lies_in_the_second_turn(gpu, caps):
    from rocco_amd.readtracks import AlignmentFileRecords, alignment_mapped_read_count_from_records, record_flag_facts_device

    tracks = lt.flag_facts_case(caps, descent=False)
    want = [int(np.count_nonzero((f[3] & 4) == 0)) for f in tracks]
    assert want[1] == 0 and 0 < want[0] < len(tracks[0][0]) and 0 < want[2] < 500
    mapped, unsorted = record_flag_facts_device([to_records(f) for f in tracks])
    assert mapped == want and unsorted == [0, 0, 0]  # (the step down from the first track's last pos to the third's first is none)
    contigs = [("a", 2 ** 30), ("b", 2 ** 30), ("c", 2 ** 30)]
    plain = (contigs, {name: dict(zip(SEVEN, f)) for (name, _), f in zip(contigs, tracks)})
    file = AlignmentFileRecords(contigs, {name: to_records(f) for (name, _), f in zip(contigs, tracks)})
    for exclude in ((), ("c",)):
        assert alignment_mapped_read_count_from_records(file, exclude) == fragment_expected.mapped_read_count(plain, exclude)
    descending = lt.flag_facts_case(caps, descent=True)
    mapped, unsorted = record_flag_facts_device([to_records(f) for f in descending])
    assert mapped == want and unsorted == [1, 0, 0]


# ---- template lengths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_second_turn", [True, False])
def test_fragment_length_of_a_paired_file_whose_templates_lie_in_one_turn(gpu, caps, in_second_turn):
    from rocco_amd.readtracks import AlignmentFileRecords, alignment_fragment_length_from_records

    contigs, records = lt.template_file(caps, in_second_turn)
    proper = np.flatnonzero(records["a"]["flag"] & 2)
    turn = caps["fragment_max_grid"] * caps["fragment_threads"]
    assert (proper.min() >= turn + 100) if in_second_turn else (proper.max() < turn)
    details = {}
    want = fragment_expected.fragment_length((contigs, records), details, flag_exclude=1024, max_iterations=1000)
    assert details["paired"] and details["templates"] > 500 and details["min_insert"] == 50 and 50 < want < 1000
    file = AlignmentFileRecords(contigs, {n: to_records([r[f] for f in SEVEN[:6]], qlen=r["qlen"]) for n, r in records.items()})
    assert alignment_fragment_length_from_records(file, flag_exclude=1024, max_iterations=1000) == want


# ---- chunk density -----------------------------------------------------------------------------------------------------
def test_chunk_density_with_a_pile_and_a_sparse_stretch_in_the_second_turn(gpu, caps):
    from rocco_amd.readtracks import fragment_block_centers_device

    pos, flag, contig_length, flag_exclude, turn = lt.density_case(caps)
    n = pos.shape[0]
    zeros = np.zeros(n, dtype=np.int32)
    records = to_records((pos, pos + 50, zeros, flag, np.full(n, 30, np.uint8), np.zeros(n, np.uint8)))
    want = fragment_expected.chunk_density(pos, flag, contig_length, flag_exclude, lt.DENSITY_BLOCK, lt.DENSITY_CHUNK)
    order = fragment_expected.ranking(want)
    centers = fragment_expected.pick_centers(want, order, lt.DENSITY_BLOCK, lt.DENSITY_CHUNK, 1000)
    pile_cell = int(pos[turn]) // lt.DENSITY_CHUNK
    assert abs(int(centers[0]) - pile_cell) <= 11 and int(want.max()) > 2000  # the densest window holds the pile of the second turn
    (got_centers,), (density,), (rank,) = fragment_block_centers_device([records], [contig_length], flag_exclude, 1000, lt.DENSITY_BLOCK,
                                                                        lt.DENSITY_CHUNK, return_density=True)
    assert np.array_equal(density.cpu().numpy(), want)
    assert np.array_equal(rank.cpu().numpy(), order)
    assert np.array_equal(got_centers, centers)


# ---- the BAM walk and the record fields --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bam(gpu, caps):
    import torch

    sizes = lt.bam_sizes(caps)
    data, entry0, offsets, want = lt.bam_stream(sizes["records"])
    n = offsets.size
    lt.bam_sample_agrees_with_the_sequential_statement(data, entry0, offsets, want, 0, 12000)
    lt.bam_sample_agrees_with_the_sequential_statement(data, entry0, offsets, want, n - 8000, n)  # (the contig's end and the unplaced records)
    return dict(data=data, entry0=entry0, offsets=offsets, want=want, bytes_t=torch.from_numpy(data).to(gpu), sizes=sizes)


def _walked(bam, caps, segment_bytes, guess_mode):
    from rocco_amd import bam as reader

    data, offsets = bam["data"], bam["offsets"]
    got, report = reader.walk_records_device(bam["bytes_t"], bam["entry0"], 3, segment_bytes, guess_mode=guess_mode, want_segment_entries=True)
    assert report["error"] == 0 and report["error_offset"] == -1 and report["end_offset"] == data.size
    assert report["records"] == offsets.size and report["segments"] == -(-data.size // segment_bytes)
    assert np.array_equal(got.cpu().numpy(), offsets)
    truth = lt.bam_true_entries(offsets, data.size, segment_bytes)
    assert np.array_equal(report["segment_entries"].cpu().numpy(), truth)
    return got, report, truth


@pytest.mark.parametrize("guess_mode", [1, 0])
def test_bam_walk_of_more_segments_than_a_turn_and_fields_of_more_records(gpu, caps, bam, guess_mode):
    """S = 64: the walk and the emit are in their second turn (and the guess far past its own); every offset and, from the
    walk's own offsets, all eight arrays."""
    from rocco_amd import bam as reader

    S = 64
    assert -(-bam["data"].size // S) > caps["bam_max_grid"] * caps["bam_threads"] < bam["offsets"].size
    got, report, truth = _walked(bam, caps, S, guess_mode)
    if guess_mode == 0:  # every segment behind entry0's guessed its first byte: the repair did the rest (tests/test_gpu_bam_records.py)
        seg0 = bam["entry0"] // S
        on_boundary = int(np.count_nonzero(truth[seg0 + 1:] == np.arange(seg0 + 1, truth.size) * S))
        assert report["repair_rounds"] == int(np.count_nonzero(truth[seg0 + 1:] >= 0)) - on_boundary
    fields, firsts, (code, record) = reader.record_fields_device(bam["bytes_t"], got, 3)
    assert (code, record) == (0, -1)
    for name, dtype in bx.FIELDS:
        a = fields[name].cpu().numpy()
        a = a.view(np.uint16) if name == "flag" else a
        assert a.dtype == dtype and np.array_equal(a, bam["want"][name]), name
    assert firsts == bx.contig_first(bam["want"]["tid"], 3).tolist()
    assert firsts[3] == bam["offsets"].size - 1500 and firsts[1] > 0


def test_bam_guess_past_its_cap_with_the_walk_inside_its_first_turn(gpu, caps, bam):
    S = 4096
    segments = -(-bam["data"].size // S)
    assert caps["bam_max_grid"] < segments < caps["bam_max_grid"] * caps["bam_threads"]
    _, report, _ = _walked(bam, caps, S, 1)
    assert report["wrong_guesses"] == 0 and report["repair_rounds"] == 0  # (no decoy in this stream: every guess is a record start)


def test_bam_stream_cut_inside_a_record_of_the_second_turn(gpu, caps, bam):
    from rocco_amd import bam as reader

    offsets = bam["offsets"]
    r = bam["sizes"]["first_record_of_second_turn"] + 411
    cut = int(offsets[r]) + 30
    assert r < offsets.size and cut < int(offsets[r + 1]) and int(offsets[r]) // 64 > caps["bam_max_grid"] * caps["bam_threads"]
    want_offsets, behind, why, where = bx.walk(bam["data"][int(offsets[r - 50]): cut].tobytes(), 0)  # (the statement, on the last 50 records)
    assert (why, where - behind, want_offsets.size) == (bx.ERR_TRUNCATED, 0, 50) and where + int(offsets[r - 50]) == int(offsets[r])
    got, report = reader.walk_records_device(bam["bytes_t"][:cut], bam["entry0"], 3, 64)
    assert report["error"] == bx.ERR_TRUNCATED and report["error_offset"] == int(offsets[r]) == report["end_offset"]
    assert report["records"] == r and np.array_equal(got.cpu().numpy(), offsets[:r])
    with pytest.raises(ValueError, match=rf"record {r} at byte {int(offsets[r])} of the inflated stream"):
        reader.decode_records_device(bam["bytes_t"][:cut], bam["entry0"], 3, 64, name="cut.bam")
