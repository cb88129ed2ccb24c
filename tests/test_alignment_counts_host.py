"""Row f5 without a GPU: the NumPy statement of the counting arithmetic (tests/alignment_counts_expected.py) equals every
fixture the reference's compiled counter and its own get_bam_chrom_reads wrote (tests/golden/alignment_count_vectors.*,
made by tests/golden/make_golden_alignment_counts.py), and the host side of rocco_amd.readtracks validates its inputs."""
import json
import logging
import os

import numpy as np
import pytest

import alignment_counts_expected as expected
from rocco_amd import readtracks as rt
from rocco_amd.readtracks import AlignmentRecords

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("pos", "end", "isize", "flag", "mapq", "mate_same")


@pytest.fixture(scope="module")
def gold():
    arrays = np.load(os.path.join(GOLDEN, "alignment_count_vectors.npz"))
    with open(os.path.join(GOLDEN, "alignment_count_vectors.json"), encoding="utf-8") as handle:
        return arrays, json.load(handle)


def records_of(arrays, key, contig):
    return tuple(arrays[f"f_{key}_{contig}_{field}"] for field in FIELDS)


def test_fixture_covers_what_it_must(gold):
    arrays, meta = gold
    assert 30 <= len(meta["count"]) <= 60
    steps = {c["step"] for c in meta["count"]}
    assert {1, 10, 50, 200} <= steps
    assert {c["options"].get("extend_bp", 0) for c in meta["count"]} >= {0, 150, 1000}
    assert any(c["prefill"] for c in meta["count"]) and any(c["length"] == 1 for c in meta["count"])
    assert any(meta["files"][c["file"]][c["contig"]] == 0 for c in meta["count"])
    assert max(max(v.values()) for v in meta["files"].values()) >= 20000
    flags = arrays["f_main_chrT_flag"]
    for bit in (1, 2, 4, 8, 16, 64, 128, 256, 1024):
        assert (flags & bit).any() and not (flags & bit).all()
    assert (arrays["f_main_chrT_end"] - arrays["f_main_chrT_pos"] == 1).any()          # a zero-length alignment
    assert (arrays["f_main_chrT_end"] > 100000).any()                                  # over the contig's end
    assert (arrays["f_main_chrT_mate_same"] == 0).any()
    assert ((arrays["f_main_chrT_isize"] > 0).any() and (arrays["f_main_chrT_isize"] < 0).any())


def test_counts_equal_the_reference(gold):
    arrays, meta = gold
    for c in meta["count"]:
        into = None
        if c["prefill"]:
            into = (np.arange(c["length"]) % c["prefill"]).astype(np.float32)
        got = expected.count_region(*records_of(arrays, c["file"], c["contig"]), c["start"], c["end"], c["step"], c["read_length"],
                                    length=c["length"], into=into, **c["options"])
        want = arrays[f"c_{c['name']}_counts"]
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), c["name"]


def test_pile_up_and_filters_are_visible_in_the_fixture(gold):
    arrays, meta = gold
    assert arrays["c_step1_pileup_counts"].max() >= 2000
    assert arrays["c_single_bin_counts"].shape == (1,)
    assert arrays["c_empty_contig_counts"].max() == 0
    assert not np.array_equal(arrays["c_paired_default_counts"], arrays["c_paired_min_template_set_counts"])
    assert not np.array_equal(arrays["c_paired_no_insert_limit_counts"], arrays["c_paired_read_length_fallback_counts"])
    # a shift never brings in a read the iterator did not yield: the region beside the pile-up stays (nearly) empty
    assert arrays["c_shift_brings_nothing_in_counts"].max() < 100


def test_ranges_equal_the_reference(gold):
    arrays, meta = gold
    seen = set()
    for r in meta["range"]:
        pos, end, _, flag, _, _ = records_of(arrays, r["file"], r["contig"])
        assert expected.chrom_range(pos, end, flag, r["chrom_len"], r["flag_exclude"]) == (r["start"], r["end"]), r
        seen.add((r["start"] > 0, r["end"] > 0))
    assert (True, False) in seen and (False, False) in seen  # a start without an end; nothing at all
    pos, end, _, flag, _, _ = records_of(arrays, "main", "chrT")
    keep = (flag & 3844) == 0
    assert expected.chrom_range(pos, end, flag, 100000, 3844)[1] != int(end[keep].max())  # the last end, not the largest


def test_tail_equals_the_reference(gold):
    arrays, meta = gold
    assert {t["kwargs"].get("round_digits", 5) for t in meta["tail"]} >= {0, 2, 5}
    for t in meta["tail"]:
        kw = {k: v for k, v in t["kwargs"].items() if k in ("min_mapping_score", "flag_include", "flag_exclude", "center_reads",
                                                             "const_scale", "round_digits", "scale_by_step")}
        got_i, got_v = expected.bam_chrom_reads(*records_of(arrays, t["file"], t["contig"]), t["chrom_size"], t["step"], t["metadata"],
                                                **kw)
        if t.get("none"):
            assert got_i is None and got_v is None, t["name"]
            continue
        want_i, want_v = arrays[f"t_{t['name']}_intervals"], arrays[f"t_{t['name']}_values"]
        assert str(got_i.dtype) == t["intervals_dtype"] and str(got_v.dtype) == t["values_dtype"] == "float64"
        assert got_i.tobytes() == want_i.tobytes() and got_v.tobytes() == want_v.tobytes(), t["name"]


def test_half_way_values_are_in_the_fixture(gold):
    arrays, meta = gold
    v = arrays["t_round0_half_way_values"]
    assert np.all(v == np.rint(v)) and (v % 2 == 0).sum() > (v % 2 == 1).sum()  # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2


def test_scale_factor_equals_the_reference(gold):
    _, meta = gold
    for s in meta["scale"]:
        got = rt._compute_native_scale_factor(s["norm_method"], s["effective_genome_size"], s["step"], s["mapped_reads"],
                                              s["norm_read_length"], s["scale_factor"])
        assert got == s["scale"], s
    for t in meta["tail"]:  # ... and the scale inside every recorded metadata dict
        call, native = t["kwargs"], t["native"]
        length = native["read_length"]
        if t["metadata"]["paired_end_mode"]:
            length = native["fragment_length"]
        elif t["metadata"]["resolved_extend_bp"] > 0:
            length = t["metadata"]["resolved_extend_bp"]
        got = rt._compute_native_scale_factor(call.get("norm_method", "RPGC"), 2.7e9, t["step"], native["mapped_reads"], length,
                                              call.get("scale_factor", 1.0))
        assert got == t["metadata"]["norm_scale"], t["name"]
    with pytest.raises(ValueError, match="Effective genome size must be positive"):
        rt._compute_native_scale_factor("RPGC", -1, 50, 10, 50)
    with pytest.raises(ValueError, match="Normalization method must be one of"):
        rt._compute_native_scale_factor("TPM", 1e9, 50, 10, 50)


def test_alignment_records_validation():
    n = 5
    good = dict(pos=np.arange(n), end=np.arange(n) + 50, isize=np.zeros(n, dtype=np.int64), flag=np.full(n, 16),
                mapq=np.full(n, 30), mate_same=np.ones(n, dtype=bool))
    r = AlignmentRecords(**good)
    assert len(r) == n and [getattr(r, f).dtype for f in FIELDS] == [np.int32, np.int32, np.int32, np.uint16, np.uint8, np.uint8]
    assert sum(getattr(r, f).nbytes for f in FIELDS) == 16 * n
    assert len(AlignmentRecords.from_numpy(*(np.zeros(0, dtype=np.int64),) * 6)) == 0
    with pytest.raises(ValueError, match=r"2\*\*31"):
        AlignmentRecords(**dict(good, end=np.array([50, 51, 52, 53, 2**31])))
    AlignmentRecords(**dict(good, end=np.array([50, 51, 52, 53, 2**31 - 1])))
    with pytest.raises(ValueError, match=r"2\*\*31"):
        AlignmentRecords(**dict(good, pos=np.array([-1, 1, 2, 3, 4])))
    with pytest.raises(TypeError, match="must hold integers"):
        AlignmentRecords(**dict(good, pos=np.arange(n, dtype=np.float64)))
    with pytest.raises(ValueError, match="has 4 entries"):
        AlignmentRecords(**dict(good, mapq=np.full(4, 30)))
    with pytest.raises(ValueError, match="does not fit uint16"):
        AlignmentRecords(**dict(good, flag=np.full(n, 70000)))
    with pytest.raises(ValueError, match="does not fit uint8"):
        AlignmentRecords(**dict(good, mapq=np.full(n, 256)))
    with pytest.raises(ValueError, match="does not fit int32"):
        AlignmentRecords(**dict(good, isize=np.full(n, 2**31)))
    with pytest.raises(ValueError, match="one-dimensional"):
        AlignmentRecords(**dict(good, pos=np.zeros((n, 1), dtype=np.int64)))


def test_count_window_and_options():
    assert rt._count_window(1237, 98761, 100000, 50) == expected.count_window(1237, 98761, 100000, 50) == (1200, 98800)
    assert rt._count_window(99990, 100147, 100000, 200) == (99800, 100000)
    assert rt._count_window(0, 1, 30, 50) == (0, 30)
    o = rt._count_options(50)
    assert (o.max_insert_size, o.min_template_length, o.shift_fwd, o.shift_rev, o.one_read_per_bin) == (1000, -1, 0, 0, 0)
    with pytest.raises(ValueError, match="only `coverage`"):
        rt._count_options(50, count_mode="cutsite")
    with pytest.raises(TypeError):
        rt._count_options(50, barcode="x")


def test_the_exactness_guard_names_its_limit():
    rt._check_exact_counts([0, 3000, 2**24])  # at the limit float32 still holds every integer
    with pytest.raises(RuntimeError, match=r"track 1 reach 16777217, beyond 2\*\*24 = 16777216"):
        rt._check_exact_counts([5, 2**24 + 1])


def test_the_stub_points_to_the_new_function():
    with pytest.raises(RuntimeError, match="bam_chrom_reads_from_records"):
        rt.get_bam_chrom_reads("a.bam")
    import rocco_amd

    for name in ("AlignmentRecords", "count_alignment_records_batch_device", "count_alignment_region_from_records",
                 "alignment_chrom_range_from_records", "bam_chrom_reads_from_records", "bam_chrom_reads_from_records_batch"):
        assert hasattr(rocco_amd, name)
