"""Row f7 on the GPU: decoded records of whole files -> the reference's count metadata (rocco_amd/csrc/fragment_length.hip
behind rocco_amd.readtracks) against everything the reference's compiled probes and its own ``_get_bam_count_metadata`` /
``get_bam_chrom_reads`` wrote (tests/golden/fragment_length_vectors.*), integer for integer, dict for dict, log line for log
line, and against the NumPy statement of the same arithmetic (tests/fragment_length_expected.py, pinned to those fixtures
by tests/test_fragment_length_host.py) at the sizes where the kernels can go wrong: lag counts across a wavefront and across
a workgroup's waves, scores compared by bit pattern, ties, empty strands, density pile-ups and contig ends."""
import json
import logging
import os

import numpy as np
import pytest

import fragment_length_expected as expected

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = expected.FIELDS[:6]


def to_records(fields):
    from rocco_amd.readtracks import AlignmentRecords

    return AlignmentRecords(*[fields[f] for f in SIX], qlen=fields["qlen"])


def to_file(contigs, records, name=""):
    from rocco_amd.readtracks import AlignmentFileRecords

    return AlignmentFileRecords(contigs, {n: to_records(r) for n, r in records.items()}, name=name)


@pytest.fixture(scope="module")
def gold():
    arrays = np.load(os.path.join(GOLDEN, "fragment_length_vectors.npz"))
    with open(os.path.join(GOLDEN, "fragment_length_vectors.json"), encoding="utf-8") as handle:
        meta = json.load(handle)
    plain, files = {}, {}
    for key, described in meta["files"].items():
        contigs = [(name, length) for name, length in described["contigs"]]
        plain[key] = (contigs, {name: {f: arrays[f"f_{key}_{name}_{f}"] for f in expected.FIELDS} for name, _ in contigs})
        files[key] = to_file(*plain[key], name="{file}")
    return arrays, meta, plain, files


def make_track(rng, n, span, dense=(1000, 1300), max_length=80):
    """n random records, half of them in a dense cluster, both strands, some unmapped / duplicate, position-sorted."""
    pos = np.sort(np.concatenate([rng.integers(0, span - max_length, size=n - n // 2), rng.integers(dense[0], dense[1], size=n // 2)]))
    flag = np.where(rng.random(n) < 0.5, 16, 0) | np.where(rng.random(n) < 0.05, 4, 0) | np.where(rng.random(n) < 0.05, 1024, 0)
    length = rng.integers(1, max_length, size=n)
    return {"pos": pos.astype(np.int32), "end": (pos + length).astype(np.int32), "isize": np.zeros(n, dtype=np.int32),
            "flag": flag.astype(np.uint16), "mapq": np.full(n, 30, dtype=np.uint8), "mate_same": np.zeros(n, dtype=np.uint8),
            "qlen": length.astype(np.int32)}


def block_track(fwd_at, rev_at, length=10):
    """Records whose forward 5' ends fall on ``fwd_at`` and reverse 5' ends on ``rev_at`` (positions, repeated as often as
    wanted): forward reads start there, reverse reads end just behind."""
    fwd_at, rev_at = np.asarray(fwd_at, dtype=np.int64), np.asarray(rev_at, dtype=np.int64)
    rev_len = np.minimum(length, rev_at + 1)
    pos = np.concatenate([fwd_at, rev_at + 1 - rev_len])
    end = np.concatenate([fwd_at + length, rev_at + 1])
    flag = np.concatenate([np.zeros(fwd_at.size, dtype=np.int64), np.full(rev_at.size, 16)])
    order = np.argsort(pos, kind="stable")
    n = pos.size
    return {"pos": pos[order].astype(np.int32), "end": end[order].astype(np.int32), "isize": np.zeros(n, dtype=np.int32),
            "flag": flag[order].astype(np.uint16), "mapq": np.full(n, 30, dtype=np.uint8), "mate_same": np.zeros(n, dtype=np.uint8),
            "qlen": (end - pos)[order].astype(np.int32)}


def check_blocks(track, starts, block_size, min_lag, max_insert, lag_step, flag_exclude=0):
    from rocco_amd.readtracks import strand_xcorr_blocks_device

    got = strand_xcorr_blocks_device([to_records(track)], [0] * len(starts), list(starts), [min_lag], flag_exclude, block_size,
                                     max_insert, lag_step)
    want = [expected.xcorr_block(track, int(s), block_size, flag_exclude, min_lag, max_insert, lag_step) for s in starts]
    assert got[0].tolist() == [w[0] for w in want]
    assert got[2].tolist() == [w[2] for w in want] and got[3].tolist() == [w[3] for w in want]
    assert got[1].tobytes() == np.asarray([w[1] for w in want], dtype=np.float64).tobytes()  # the scores by bit pattern
    return got, want


def test_probes_equal_the_reference(gpu, gold):
    from rocco_amd import readtracks as rt

    _, meta, _, files = gold
    for r in meta["paired"]:
        assert int(rt.is_alignment_paired_end_from_records(files[r["file"]], r["max_reads"])) == r["paired"], r
    for r in meta["readlen"]:
        if r["error"] is not None:
            with pytest.raises(RuntimeError, match=r["error"]):
                rt.alignment_read_length_from_records(files[r["file"]], r["min_reads"], r["max_iterations"], r["flag_exclude"])
        else:
            assert rt.alignment_read_length_from_records(files[r["file"]], r["min_reads"], r["max_iterations"],
                                                         r["flag_exclude"]) == r["read_length"], r
    for r in meta["mapped"]:
        assert rt.alignment_mapped_read_count_from_records(files[r["file"]], r["exclude"]) == (r["mapped"], r["unmapped"]), r


def test_fragment_lengths_equal_the_reference(gpu, gold):
    """Every fixture scenario: one batch call per parameter set over the files it was recorded for."""
    from rocco_amd.readtracks import alignment_fragment_length_from_records_batch

    _, meta, _, files = gold
    by_parameters = {}
    for r in meta["fraglen"]:
        by_parameters.setdefault(json.dumps(r["params"], sort_keys=True), []).append(r)
    assert len(by_parameters) >= 60
    for text, scenarios in by_parameters.items():
        got = alignment_fragment_length_from_records_batch([files[r["file"]] for r in scenarios], **json.loads(text))
        assert got == [r["fragment_length"] for r in scenarios], (text, [r["file"] for r in scenarios])


def test_device_resident_records_give_the_same(gpu, gold):
    from rocco_amd.readtracks import AlignmentFileRecords, alignment_fragment_length_from_records, bam_count_metadata_from_records

    _, meta, _, files = gold
    for key in ("se_peaks", "pe_b", "mixed"):
        on_device = AlignmentFileRecords(files[key].contigs, {n: r.to("cuda") for n, r in files[key].records.items()}, name="{file}")
        wanted = {json.dumps(r["params"], sort_keys=True): r["fragment_length"] for r in meta["fraglen"] if r["file"] == key}
        assert alignment_fragment_length_from_records(on_device) == wanted["{}"]
        assert alignment_fragment_length_from_records(on_device, max_iterations=4096) == wanted['{"max_iterations": 4096}']
        scenario = next(r for r in meta["metadata"] if r["file"] == key and r["call"]["extend_reads"] == 0)
        assert bam_count_metadata_from_records(on_device, **scenario["call"]) == scenario["metadata"]


def test_count_metadata_equals_the_reference(gpu, gold, caplog):
    from rocco_amd.readtracks import bam_count_metadata_from_records, bam_count_metadata_from_records_batch

    _, meta, _, files = gold
    for r in meta["metadata"]:
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="rocco_amd.readtracks"):
            if r["error"] is not None:
                with pytest.raises(RuntimeError, match=r["error"]):
                    bam_count_metadata_from_records(files[r["file"]], **r["call"])
                continue
            got = bam_count_metadata_from_records(files[r["file"]], **r["call"])
        assert got == r["metadata"] and "threads" not in got, r
        assert [[rec.levelname, rec.getMessage()] for rec in caplog.records if rec.name == "rocco_amd.readtracks"] == r["log"], r
    call = dict(step=50, norm_method="RPGC", effective_genome_size=2.7e9, ignore_for_norm=None, flag_exclude=0, extend_reads=0)
    keys = [key for key in files if key != "empty"]
    wanted = {r["file"]: r["metadata"] for r in meta["metadata"] if r["call"] == dict(call, scale_factor=1.0)}
    assert bam_count_metadata_from_records_batch([files[key] for key in keys], **call) == [wanted[key] for key in keys]


def test_metadata_feeds_the_counting(gpu, gold):
    """`bam_count_metadata_from_records` -> `bam_chrom_reads_from_records` gives what the reference's own
    ``get_bam_chrom_reads`` wrote for the file."""
    from rocco_amd.readtracks import bam_chrom_reads_from_records, bam_count_metadata_from_records

    arrays, meta, _, files = gold
    for r in meta["chrom_reads"]:
        k = r["kwargs"]
        file = files[r["file"]]
        metadata = bam_count_metadata_from_records(file, r["step"], k["norm_method"], k["effective_genome_size"], k["ignore_for_norm"],
                                                   flag_exclude=k["flag_exclude"], extend_reads=k["extend_reads"],
                                                   scale_factor=k["scale_factor"])
        intervals, values = bam_chrom_reads_from_records(
            file.records[r["contig"]], dict(file.contigs)[r["contig"]], r["step"], metadata, min_mapping_score=k["min_mapping_score"],
            flag_include=k["flag_include"], flag_exclude=k["flag_exclude"], center_reads=k["center_reads"], const_scale=k["const_scale"],
            round_digits=k["round_digits"], scale_by_step=k["scale_by_step"], bam_file="{file}", chromosome=r["contig"])
        assert np.array_equal(intervals, arrays[f"r_{r['name']}_intervals"]), r["name"]
        assert values.tobytes() == arrays[f"r_{r['name']}_values"].tobytes(), r["name"]


def test_batch_equals_single_calls(gpu, gold):
    from rocco_amd.readtracks import alignment_fragment_length_from_records, alignment_fragment_length_from_records_batch

    _, _, _, files = gold
    three = [files["se_peaks"], files["pe_a"], files["se_dense"]]
    for parameters in (dict(), dict(block_size=257, lag_step=1, rolling_chunk_size=100, early_exit=4, max_iterations=3)):
        together = alignment_fragment_length_from_records_batch(three, **parameters)
        assert together == [alignment_fragment_length_from_records(f, **parameters) for f in three]
    assert alignment_fragment_length_from_records_batch(three)[0] > 100


@pytest.mark.parametrize("n_lags, block_size, min_lag, lag_step", [(1, 64, 50, 5), (63, 257, 10, 1), (64, 257, 10, 1), (65, 257, 10, 1),
                                                                   (200, 5000, 20, 5), (300, 1000, 1, 1), (9, 64, 1, 7)])
def test_blocks_equal_the_statement_bit_for_bit(gpu, n_lags, block_size, min_lag, lag_step):
    """Lag counts of 1, 63, 64, 65 and 200: the reduction inside a wavefront, across a workgroup's waves and (300) over a
    thread's second lag."""
    max_insert = min_lag + (n_lags - 1) * lag_step
    track = make_track(np.random.default_rng(100 + n_lags), 4000, 30000, max_length=min(80, block_size // 2))
    starts = [0, 990, 1000, 1100, 1234, 30000 - block_size, 7000]
    got, want = check_blocks(track, starts, block_size, min_lag, max_insert, lag_step)
    assert sum(1 for w in want if w[0] > 0) >= 3 and len({w[0] for w in want}) >= 2
    assert all((w[0] - min_lag) % lag_step == 0 and w[0] <= max_insert for w in want if w[0] > 0)
    check_blocks(track, starts[:4], block_size, min_lag, max_insert, lag_step, flag_exclude=1024 | 4)


def test_largest_block_size_and_the_one_beyond(gpu):
    from rocco_amd.readtracks import (AlignmentFileRecords, alignment_fragment_length_from_records, fragment_length_shape,
                                      strand_xcorr_blocks_device)

    limit = fragment_length_shape()["max_block_size"]
    assert limit >= 5000 and limit * 8 + 256 <= 160 * 1024
    track = make_track(np.random.default_rng(7), 3000, limit + 500, dense=(limit - 400, limit - 100))
    check_blocks(track, [0, 500], limit, 40, 60, 5)
    with pytest.raises(ValueError, match=str(limit)):
        strand_xcorr_blocks_device([to_records(track)], [0], [0], [40], 0, limit + 1, 60, 5)
    file = AlignmentFileRecords([("c", 4 * limit)], {"c": to_records(track)}, name="big.bam")
    with pytest.raises(ValueError, match=str(limit)):
        alignment_fragment_length_from_records(file, block_size=limit + 1)


def test_equal_scores_keep_the_smaller_lag(gpu):
    """Duplicate structure: forward piles at 14 and 15, reverse piles at 23, 38, 45 and 48 of a 64-bp block (32 reads each:
    both means are whole numbers, so every product and every partial sum is exact) -- lags 8 and 24 reach the same score."""
    track = block_track(np.repeat([14, 15], 32), np.repeat([23, 38, 45, 48], 32))
    f = np.bincount(np.repeat([14, 15], 32), minlength=64) - 1.0
    r = np.bincount(np.repeat([23, 38, 45, 48], 32), minlength=64) - 2.0
    scores = expected.lag_scores(f, r, np.arange(5, 60))
    assert np.flatnonzero(scores == scores.max()).tolist() == [8 - 5, 24 - 5] and scores[3].tobytes() == scores[19].tobytes()
    got, _ = check_blocks(track, [0], 64, 5, 59, 1)
    assert got[0].tolist() == [8] and got[1].tolist() == [880.0]
    got, _ = check_blocks(track, [0], 64, 24, 59, 1)  # (without the smaller one in range: the larger)
    assert got[0].tolist() == [24]


def test_flat_reverse_strand_scores_zero(gpu):
    """One reverse 5' end on every position of a 64-bp block: every centred value is 0, every score 0.0, no candidate."""
    from rocco_amd.readtracks import AlignmentFileRecords, alignment_fragment_length_from_records

    track = block_track(np.repeat([3, 9, 20], 5), np.arange(64), length=1)
    got, want = check_blocks(track, [0], 64, 1, 63, 1)
    assert want[0][:2] == (1, 0.0) and got[2].tolist() == [15] and got[3].tolist() == [64]
    assert not (got[0][0] > 0 and got[1][0] != 0.0)
    file = AlignmentFileRecords([("c", 64)], {"c": to_records(track)})
    assert alignment_fragment_length_from_records(file, block_size=64, lag_step=1, fallback=147) == 147
    assert alignment_fragment_length_from_records(file, block_size=64, lag_step=1) == 0


def test_nine_and_ten_reads_on_a_strand(gpu):
    rev = np.repeat([150, 160, 170], 8)
    for fwd_reads, candidate in ((9, False), (10, True)):
        track = block_track(np.repeat([20], fwd_reads), rev)
        got, want = check_blocks(track, [0], 257, 30, 200, 5)
        assert got[2].tolist() == [fwd_reads] and (got[0][0] > 0) == candidate
    track = block_track(np.repeat([20], 12), rev[:9])
    got, _ = check_blocks(track, [0], 257, 30, 200, 5)
    assert got[3].tolist() == [9] and got[0].tolist() == [-1] and got[1].tolist() == [0.0]


def density_case(track, contig_length, block_size, chunk, max_iterations, flag_exclude=0):
    from rocco_amd.readtracks import fragment_block_centers_device

    centers, density, rank = fragment_block_centers_device([to_records(track)], [contig_length], flag_exclude, max_iterations, block_size,
                                                           chunk, return_density=True)
    want = expected.chunk_density(track["pos"], track["flag"], contig_length, flag_exclude, block_size, chunk)
    order = expected.ranking(want)
    if contig_length < block_size:
        assert density[0].numel() == 0 and rank[0].numel() == 0 and centers[0].size == 0
        return want, order, centers[0]
    assert density[0].cpu().numpy().tolist() == want.tolist()
    assert rank[0].cpu().numpy().tolist() == order.tolist()
    assert centers[0].tolist() == expected.pick_centers(want, order, block_size, chunk, max_iterations).tolist()
    return want, order, centers[0]


def test_density_ranking_and_centres(gpu):
    from rocco_amd.readtracks import fragment_length_shape

    shape = fragment_length_shape()
    rng = np.random.default_rng(11)
    # several thousand records in one chunk (four trips of a workgroup; one record in twenty is unmapped and not counted);
    # records in the first and in the last chunk; a contig that ends inside a chunk
    contig = 100 * 250 - 70
    pos = np.sort(np.concatenate([rng.integers(5000, 5250, size=4 * shape["density_records"] + 77), rng.integers(0, 250, size=30),
                                  rng.integers(contig - 180, contig, size=20), rng.integers(0, contig, size=500)]))
    track = make_track(rng, pos.size, contig)
    track["pos"], track["end"] = pos.astype(np.int32), (pos + 30).astype(np.int32)
    want, _, centers = density_case(track, contig, 5000, 250, 1000)
    assert want.max() > 3 * shape["density_records"] and want[0] > 0 and want[-1] > 0 and centers.size >= 3
    density_case(track, contig, 5000, 250, 2, flag_exclude=16)
    # a sparse track: cells far beyond one LDS window of the workgroup's first record
    far = make_track(rng, 600, 250 * (4 * shape["density_window"]), dense=(0, 250 * (4 * shape["density_window"]) - 100))
    density_case(far, 250 * (4 * shape["density_window"]), 5000, 250, 50)
    density_case(far, 250 * (4 * shape["density_window"]), 64, 1, 7)
    # fewer chunks than the window is wide: every window is the whole contig, every value ties, the index decides; centre 0
    # marks the cells 0 .. 10 (the window's unclamped start is -10), so chunk 11 is the second and last centre
    want, order, centers = density_case(track, 5000, 5000, 250, 1000)  # (20 chunks, a window of 21)
    assert want.size == 20 and len(set(want.tolist())) == 1 and order.tolist() == list(range(20)) and centers.tolist() == [0, 11]
    assert density_case(track, 4999, 5000, 250, 1000)[0].size == 20  # (shorter than a block: the reference skips the contig)
    # a window of one chunk (rolling_chunk_size beyond block_size) with equal counts in many chunks: ties broken by index
    tied = block_track(np.repeat(np.arange(10) * 7000 + 5, 4), np.repeat(np.arange(10) * 7000 + 90, 4))
    want, order, centers = density_case(tied, 70000, 5000, 7000, 6)
    assert want.tolist() == [8] * 10 and centers.tolist() == [0, 1, 2, 3, 4, 5]


def test_unsorted_track_is_refused(gpu, gold):
    from rocco_amd.readtracks import AlignmentFileRecords, alignment_fragment_length_from_records_batch

    _, _, plain, files = gold
    contigs, records = plain["se_peaks"]
    shuffled = {f: a.copy() for f, a in records["chrB"].items()}
    for f in expected.FIELDS:
        shuffled[f][[100, 300]] = shuffled[f][[300, 100]]
    bad = AlignmentFileRecords(contigs, {n: to_records(shuffled if n == "chrB" else r) for n, r in records.items()}, name="shuffled.bam")
    with pytest.raises(ValueError, match=r"shuffled\.bam on chrB"):
        alignment_fragment_length_from_records_batch([files["se_peaks"], bad])


def test_missing_query_length_is_refused(gpu, gold):
    from rocco_amd.readtracks import AlignmentFileRecords, AlignmentRecords, alignment_fragment_length_from_records, bam_count_metadata_from_records

    _, _, plain, _ = gold
    contigs, records = plain["se_peaks"]
    bare = AlignmentFileRecords(contigs, {n: AlignmentRecords(*[r[f] for f in SIX]) for n, r in records.items()}, name="bare.bam")
    with pytest.raises(ValueError, match="qlen"):
        alignment_fragment_length_from_records(bare)
    with pytest.raises(ValueError, match="qlen"):
        bam_count_metadata_from_records(bare, 50, "CPM", -1, None)
