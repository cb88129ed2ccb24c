"""Row f5 on the GPU: decoded alignment records -> binned coverage (rocco_amd/csrc/count.hip) against the fixtures the
reference's compiled counter and its own get_bam_chrom_reads wrote (tests/golden/alignment_count_vectors.*), byte for
byte, and against the NumPy statement of the same arithmetic (tests/alignment_counts_expected.py, pinned to those
fixtures by tests/test_alignment_counts_host.py) at the sizes where the kernels change path.

The counting kernel gives every workgroup `chunk` records at a time and a launch `grid` workgroups at most (further
chunks are taken by the same workgroups in turn), aggregates in an LDS window of `window` bins and scans the bins in
tiles of `tile`; the library reports the four numbers (rocco_hip_count_alignment_shape)."""
import ctypes
import json
import logging
import os

import numpy as np
import pytest

import alignment_counts_expected as expected

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("pos", "end", "isize", "flag", "mapq", "mate_same")


@pytest.fixture(scope="module")
def gold():
    arrays = np.load(os.path.join(GOLDEN, "alignment_count_vectors.npz"))
    with open(os.path.join(GOLDEN, "alignment_count_vectors.json"), encoding="utf-8") as handle:
        return arrays, json.load(handle)


@pytest.fixture(scope="module")
def shape(gpu):
    from rocco_amd import _native

    out = (ctypes.c_int * 4)()
    _native.load().rocco_hip_count_alignment_shape(out)
    chunk, grid, tile, window = (int(v) for v in out)
    assert chunk > 0 and grid > 0 and tile > 0 and window > 0
    return dict(chunk=chunk, grid=grid, tile=tile, window=window)


def fields_of(arrays, key, contig):
    return tuple(arrays[f"f_{key}_{contig}_{field}"] for field in FIELDS)


def records_of(arrays, key, contig):
    from rocco_amd.readtracks import AlignmentRecords

    return AlignmentRecords(*fields_of(arrays, key, contig))


def options_of(c):
    return dict(read_length=c["read_length"], **c["options"])


def prefill_of(c, gpu):
    import torch

    if not c["prefill"]:
        return None
    return torch.from_numpy((np.arange(c["length"]) % c["prefill"]).astype(np.float32)).to(gpu)


def test_every_count_scenario_one_track_per_call(gpu, gold):
    from rocco_amd.readtracks import count_alignment_records_batch_device, count_alignment_region_from_records

    arrays, meta = gold
    for c in meta["count"]:
        records = records_of(arrays, c["file"], c["contig"])
        before = prefill_of(c, gpu)
        (got,) = count_alignment_records_batch_device([records], [(c["start"], c["end"], c["step"])], [options_of(c)],
                                                      lengths=[c["length"]], into=None if before is None else [before])
        want = arrays[f"c_{c['name']}_counts"]
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), c["name"]
        if not c["prefill"] and c["length"] == expected.n_bins(c["start"], c["end"], c["step"]):
            again = count_alignment_region_from_records(records, c["start"], c["end"], c["step"], c["read_length"], **c["options"])
            assert isinstance(again, np.ndarray) and again.tobytes() == want.tobytes(), c["name"]


def test_every_range_scenario(gpu, gold):
    from rocco_amd.readtracks import alignment_chrom_range_from_records

    arrays, meta = gold
    for r in meta["range"]:
        got = alignment_chrom_range_from_records(records_of(arrays, r["file"], r["contig"]), r["chrom_len"], r["flag_exclude"])
        assert got == (r["start"], r["end"]), r


def test_count_scenarios_batched_seven_at_a_time(gpu, gold):
    """Different options, regions and record sets per track in one launch series: a workgroup that took another
    track's options or offsets would show."""
    from rocco_amd.readtracks import count_alignment_records_batch_device

    arrays, meta = gold
    cases = [c for c in meta["count"] if not c["prefill"]]
    order = np.random.default_rng(5).permutation(len(cases))
    cases = [cases[i] for i in order]
    for at in range(0, len(cases), 7):
        group = cases[at: at + 7]
        got = count_alignment_records_batch_device([records_of(arrays, c["file"], c["contig"]) for c in group],
                                                   [(c["start"], c["end"], c["step"]) for c in group],
                                                   [options_of(c) for c in group], lengths=[c["length"] for c in group])
        for c, g in zip(group, got):
            assert g.cpu().numpy().tobytes() == arrays[f"c_{c['name']}_counts"].tobytes(), (at, c["name"])


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def test_tail_scenarios_through_bam_chrom_reads_from_records(gpu, gold):
    from rocco_amd import readtracks as rt

    arrays, meta = gold
    ours = ("No mapped reads found", "No non-zero values found", "You are scaling the values by 0.")
    for t in meta["tail"]:
        kw = {k: v for k, v in t["kwargs"].items() if k in ("min_mapping_score", "flag_include", "flag_exclude", "center_reads",
                                                             "const_scale", "round_digits", "scale_by_step")}
        keep = Keep()
        rt.logger.addHandler(keep)
        try:
            got_i, got_v = rt.bam_chrom_reads_from_records(records_of(arrays, t["file"], t["contig"]), t["chrom_size"], t["step"],
                                                           t["metadata"], bam_file="{file}", chromosome=t["contig"], **kw)
        finally:
            rt.logger.removeHandler(keep)
        assert keep.messages == [m for m in t["warnings"] if m.startswith(ours)], t["name"]  # (the rest belongs to the metadata lookup)
        if t.get("none"):
            assert got_i is None and got_v is None, t["name"]
            continue
        want_i, want_v = arrays[f"t_{t['name']}_intervals"], arrays[f"t_{t['name']}_values"]
        assert str(got_i.dtype) == t["intervals_dtype"] and str(got_v.dtype) == t["values_dtype"], t["name"]
        assert got_i.tobytes() == want_i.tobytes() and got_v.tobytes() == want_v.tobytes(), t["name"]


def check_random(gpu, tracks):
    """tracks: (fields, (start, end, step), options).  One batched call against the NumPy statement."""
    from rocco_amd.readtracks import AlignmentRecords, count_alignment_records_batch_device

    got = count_alignment_records_batch_device([AlignmentRecords(*f) for f, _, _ in tracks], [r for _, r, _ in tracks],
                                               [dict(read_length=50, **o) for _, _, o in tracks])
    for k, ((f, (start, end, step), o), g) in enumerate(zip(tracks, got)):
        want = expected.count_region(*f, start, end, step, 50, **o)
        assert g.cpu().numpy().tobytes() == want.tobytes(), (k, len(f[0]), (start, end, step), o)


def test_record_counts_around_a_workgroup_share_and_a_launch_share(gpu, shape):
    rng = np.random.default_rng(11)
    sizes = [1, shape["chunk"] - 1, shape["chunk"], shape["chunk"] + 1]
    check_random(gpu, [(expected.random_records(rng, n, 40000), (0, 40000, 50), dict(extend_bp=150)) for n in sizes])
    launch = shape["chunk"] * shape["grid"]
    assert launch <= 300000
    for n in (launch - 1, launch, launch + 1):  # alone in their call: the grid is the call's
        check_random(gpu, [(expected.random_records(rng, n, 3000000), (0, 3000000, 50), dict(flag_exclude=1796, min_mapping_quality=10))])
    # ... and the share reached by several tracks together, the last one past it
    third = launch // 3
    check_random(gpu, [(expected.random_records(rng, n, 500000), (0, 500000, 10), dict(paired_end_mode=1)) for n in (third, third, third + 7, 5)])


def test_bin_counts_around_the_scan_tiles(gpu, shape):
    rng = np.random.default_rng(12)
    tile = shape["tile"]
    tracks = []
    for bins in (1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
        step = 7
        end = 1000 + bins * step - int(rng.integers(0, step))  # (ends off the grid: the last bin is short)
        assert expected.n_bins(1000, end, step) == bins
        tracks.append((expected.random_records(rng, 4000, bins * step + 2000), (1000, end, step), dict(extend_bp=int(rng.choice([0, 150])))))
    check_random(gpu, tracks)
    check_random(gpu, [(expected.random_records(rng, 3000, 80000), (0, 69999, 1), dict(one_read_per_bin=1)),
                       (expected.random_records(rng, 3000, 80000), (0, 70000, 1), {})])


def test_pile_up_in_one_bin_and_fragments_past_the_window(gpu, shape):
    rng = np.random.default_rng(13)
    n = 9 * shape["chunk"] + 3
    pile = expected.random_records(rng, n, 40, first=20000)  # every record in one 50 bp bin: LDS aggregation and its flush
    tracks = [(pile, (0, 50000, 50), {}), (pile, (0, 50000, 50), dict(one_read_per_bin=1)), (pile, (20000, 20050, 50), {})]
    # fragments longer than the window: their far end goes to global memory directly
    far = (shape["window"] + 50) * 10
    long_reads = list(expected.random_records(rng, 5000, 200000))
    long_reads[1] = (long_reads[0] + rng.integers(far, 2 * far, size=5000)).astype(np.int32)
    tracks.append((tuple(long_reads), (0, 250000, 10), {}))
    tracks.append((expected.random_records(rng, 5000, 200000), (0, 200000, 10), dict(extend_bp=far)))
    paired = list(expected.random_records(rng, 5000, 200000, paired=1.0))
    paired[2] = (paired[2].astype(np.int64) * 40).astype(np.int32)
    tracks.append((tuple(paired), (0, 200000, 10), dict(paired_end_mode=1, max_insert_size=0)))
    unsorted = tuple(a[rng.permutation(5000)] for a in expected.random_records(rng, 5000, 200000))  # no window fits: still right
    tracks.append((unsorted, (0, 200000, 10), {}))
    check_random(gpu, tracks)


def test_empty_track_between_two_others_and_records_outside_the_region(gpu, shape):
    rng = np.random.default_rng(14)
    empty = tuple(np.zeros(0, dtype=d) for d in (np.int32, np.int32, np.int32, np.uint16, np.uint8, np.uint8))
    a, b = expected.random_records(rng, 2 * shape["chunk"] + 9, 30000), expected.random_records(rng, 777, 30000)
    outside = expected.random_records(rng, 3000, 10000, first=50000)
    check_random(gpu, [(a, (0, 30000, 50), {}), (empty, (0, 30000, 50), {}), (b, (100, 29000, 10), dict(extend_bp=150)),
                       (outside, (0, 30000, 50), dict(shift_forward_strand53=-45000, shift_reverse_strand53=45000)),
                       (outside, (70000, 90000, 50), dict(extend_bp=1000)), (empty, (5, 6, 1), dict(one_read_per_bin=1))])


def reported_magnitudes(gpu, tracks, lengths=None, into=None):
    """tracks: (fields, (start, end, step), options with read_length).  What `rocco_hip_count_alignment_records_batch`
    writes to max_magnitude_out_host for one call, and the counts."""
    from rocco_amd import readtracks as rt

    cat, offsets = rt._records_on_device([rt.AlignmentRecords(*f) for f, _, _ in tracks], gpu)
    return rt._count_concatenated(cat, offsets, [r for _, r, _ in tracks], [o for _, _, o in tracks], lengths, into)


def test_reported_magnitude_of_the_pile_up_fixtures(gpu, gold):
    """The 2**24 guard rests on the per-track maximum the scan kernel reports: the largest magnitude of a difference cell
    (the one behind the last bin included) or of a running value; with one_read_per_bin the largest count."""
    arrays, meta = gold
    by_name = {c["name"]: c for c in meta["count"]}
    for name, at_least in (("step1_pileup", 2500), ("single_bin", 3000), ("one_read_per_bin_step1", 50), ("short_buffer", 1),
                           ("short_buffer_one_read", 1), ("empty_contig", 0)):
        c = by_name[name]
        f = fields_of(arrays, c["file"], c["contig"])
        want = expected.max_magnitude(*f, c["start"], c["end"], c["step"], c["read_length"], length=c["length"], **c["options"])
        assert want >= at_least, name  # (the scenario is as deep as it is meant to be)
        _, got = reported_magnitudes(gpu, [(f, (c["start"], c["end"], c["step"]), options_of(c))], lengths=[c["length"]])
        assert got == [want], name
    # into a used buffer with one_read_per_bin the sum counts as well (the reference adds 1.0f at a time there)
    import torch

    c = by_name["into_used_buffer_one_read"]
    f = fields_of(arrays, c["file"], c["contig"])
    used = np.full(c["length"], 7, dtype=np.float32)
    views, got = reported_magnitudes(gpu, [(f, (c["start"], c["end"], c["step"]), options_of(c))], lengths=[c["length"]],
                                     into=[torch.from_numpy(used).to(gpu)])
    want = expected.count_region(*f, c["start"], c["end"], c["step"], c["read_length"], length=c["length"], into=used, **c["options"])
    assert views[0].cpu().numpy().tobytes() == want.tobytes()
    alone = expected.max_magnitude(*f, c["start"], c["end"], c["step"], c["read_length"], length=c["length"], **c["options"])
    assert got == [alone + 7] and int(want.max()) == alone + 7


def test_reported_magnitudes_of_a_batch_with_a_depth_of_its_own_per_track(gpu, shape):
    """One call, another depth in every track: a maximum written to the wrong track, a scan tile left out or the cell
    behind the last bin dropped would show."""
    rng = np.random.default_rng(15)
    chunk, tile = shape["chunk"], shape["tile"]
    empty = tuple(np.zeros(0, dtype=d) for d in (np.int32, np.int32, np.int32, np.uint16, np.uint8, np.uint8))
    deep = expected.random_records(rng, 9 * chunk + 3, 40, first=20000)
    middling = expected.random_records(rng, 2 * chunk + 1, 40, first=3 * tile * 50 + 20)  # its pile lies in the fourth scan tile
    tracks = [(deep, (0, 50000, 50), {}),
              (expected.random_records(rng, 777, 30000), (0, 30000, 50), dict(extend_bp=150)),
              (deep, (0, 50000, 50), dict(one_read_per_bin=1, min_mapping_quality=30)),
              (empty, (0, 30000, 50), {}),
              (deep, (19000, 20020, 50), dict(extend_bp=400)),  # every fragment runs past the region: the cell behind the last bin
              (middling, (0, 4 * tile * 50, 50), dict(flag_exclude=1796)),
              (expected.random_records(rng, 5000, 200000), (0, 200000, 10), dict(paired_end_mode=1, max_insert_size=0))]
    want = [expected.max_magnitude(*f, *r, 50, **o) for f, r, o in tracks]
    assert want[3] == 0 and len(set(want)) == len(want) and want[0] > 4000 and want[4] > 2000, want
    cells = expected.difference_cells(*deep, 19000, 20020, 50, 50, extend_bp=400)
    assert -cells[-1] == want[4]  # (there the last cell is as large as anything before it)
    views, got = reported_magnitudes(gpu, [(f, r, dict(read_length=50, **o)) for f, r, o in tracks])
    assert got == want
    for (f, (start, end, step), o), view in zip(tracks, views):
        assert view.cpu().numpy().tobytes() == expected.count_region(*f, start, end, step, 50, **o).tobytes()


def test_batch_output_feeds_assemble_chrom_matrix(gpu, gold):
    from rocco_amd import readtracks as rt

    arrays, meta = gold
    picks = [t for t in meta["tail"] if t["step"] == 50 and t["contig"] == "chrT" and not t["kwargs"].keys() - {"norm_method", "extend_reads", "scale_factor"}]
    picks = picks[:5] + [t for t in meta["tail"] if t["name"] == "big_default"]
    records = [records_of(arrays, t["file"], t["contig"]) for t in picks]
    intervals, vals = rt.bam_chrom_reads_from_records_batch(records, 100000, 50, [t["metadata"] for t in picks])
    singles = [rt.bam_chrom_reads_from_records(r, 100000, 50, t["metadata"]) for r, t in zip(records, picks)]
    for t, i, v, (si, sv) in zip(picks, intervals, vals, singles):
        assert i.tobytes() == arrays[f"t_{t['name']}_intervals"].tobytes() == si.tobytes(), t["name"]
        assert v.tobytes() == arrays[f"t_{t['name']}_values"].tobytes() == sv.tobytes(), t["name"]
    got_common, got_matrix = rt.assemble_chrom_matrix(intervals, vals)
    want_common, want_matrix = rt.assemble_chrom_matrix([s[0] for s in singles], [s[1] for s in singles])
    assert got_common.tobytes() == want_common.tobytes() and got_matrix.tobytes() == want_matrix.tobytes()
    assert got_matrix.shape == (len(picks), got_common.size) and got_matrix.dtype == np.float64
    # a file without data has None in both lists and generate_chrom_matrix's rule leaves it out
    empty = records_of(arrays, "main", "chrE")
    i2, v2 = rt.bam_chrom_reads_from_records_batch([records[0], empty, records[1]], 100000, 50, [picks[0]["metadata"]] * 2 + [picks[1]["metadata"]])
    assert i2[1] is None and v2[1] is None and i2[0].tobytes() == intervals[0].tobytes() and v2[2].tobytes() == vals[1].tobytes()


def test_device_tensors_in(gpu, gold):
    import torch

    from rocco_amd.readtracks import AlignmentRecords, count_alignment_records_batch_device

    arrays, meta = gold
    c = next(c for c in meta["count"] if c["name"] == "big_paired")
    f = fields_of(arrays, c["file"], c["contig"])
    tensors = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu) for a in f]
    (got,) = count_alignment_records_batch_device([AlignmentRecords(*tensors)], [(c["start"], c["end"], c["step"])], [options_of(c)])
    assert got.cpu().numpy().tobytes() == arrays["c_big_paired_counts"].tobytes()
    with pytest.raises(TypeError, match="int32 tensor"):
        AlignmentRecords(tensors[0].to(torch.int64), *tensors[1:])


def test_a_device_named_without_an_index(gpu):
    """``device="cuda"`` names the current device: the same counts as with the indexed device."""
    import torch

    from rocco_amd.readtracks import AlignmentRecords, count_alignment_records_batch_device

    pos = np.arange(12, dtype=np.int64) * 37 + 5
    records = AlignmentRecords(pos, pos + 50, np.zeros(12, dtype=np.int64), np.where(np.arange(12) % 2, 16, 0), np.full(12, 30), np.zeros(12, dtype=np.int64))
    region, options = [(0, 600, 25)], [dict(read_length=50)]
    with torch.cuda.device(gpu):
        (loose,) = count_alignment_records_batch_device([records], region, options, device="cuda")
    (indexed,) = count_alignment_records_batch_device([records], region, options, device=gpu)
    assert loose.device == indexed.device == gpu and loose.shape[0] == 24 and float(indexed.sum()) > 0
    assert torch.equal(loose, indexed)
