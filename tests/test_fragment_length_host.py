"""Row f7 without a GPU: the NumPy statement of the whole-file probes (tests/fragment_length_expected.py) equals every
fixture the reference's compiled probes and its own ``_get_bam_count_metadata`` wrote (tests/golden/fragment_length_vectors.*,
made by tests/golden/make_golden_fragment_length.py), and the host side of rocco_amd.readtracks keeps its contract."""
import json
import os

import numpy as np
import pytest

import fragment_length_expected as expected
from rocco_amd import readtracks as rt
from rocco_amd.readtracks import AlignmentFileRecords, AlignmentRecords

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    arrays = np.load(os.path.join(GOLDEN, "fragment_length_vectors.npz"))
    with open(os.path.join(GOLDEN, "fragment_length_vectors.json"), encoding="utf-8") as handle:
        meta = json.load(handle)
    files = {}
    for key, described in meta["files"].items():
        contigs = [(name, length) for name, length in described["contigs"]]
        files[key] = (contigs, {name: {f: arrays[f"f_{key}_{name}_{f}"] for f in expected.FIELDS} for name, _ in contigs})
    return arrays, meta, files


@pytest.fixture(scope="module")
def caches(gold):
    return {key: {} for key in gold[2]}  # (the statement's correlated blocks, per file, shared by the scenarios)


def test_fixture_covers_what_it_must(gold):
    arrays, meta, files = gold
    assert os.path.getsize(os.path.join(GOLDEN, "fragment_length_vectors.npz")) < 1 << 20
    names = {name: length for name, length in files["se_peaks"][0]}
    top = expected.top_contigs(files["se_peaks"][0])
    assert [n for n, _ in top] == ["chrA", "chrB", "chrC"] and names["chrB"] == names["chrC"]  # the first of equals stays ahead
    assert [n for n, _ in files["se_peaks"][0]][:3] != [n for n, _ in top]                    # header order is another order
    assert min(names.values()) < 5000 and any(length < 5000 for _, length in expected.top_contigs(files["se_short"][0]))
    flags = np.concatenate([arrays[f"f_se_peaks_{n}_flag"] for n in names])
    assert (flags & 4).any() and (flags & 16).any() and (flags & 1024).any()
    qlen, span = arrays["f_se_peaks_chrA_qlen"], arrays["f_se_peaks_chrA_end"] - arrays["f_se_peaks_chrA_pos"]
    assert (qlen == 0).any() and (qlen != span).any()            # unmapped without SEQ; CIGARs whose span is not the query
    assert (arrays["f_se_noseq_chrA_qlen"] > 0).all()            # SEQ `*` everywhere: the CIGAR's length
    params = [r["params"] for r in meta["fraglen"]]
    assert {p.get("lag_step", 5) for p in params} >= {0, 1, 5, 7}
    assert {p.get("block_size", 5000) for p in params} >= {0, 10, 64, 257, 1000, 5000}
    assert {p.get("rolling_chunk_size", 250) for p in params} >= {0, 1, 100, 250, 7000}
    assert {p.get("max_iterations", 1000) for p in params} >= {0, 1, 3, 1000, 4096}
    assert {p.get("early_exit", 250) for p in params} >= {-3, 0, 1, 3, 4, 5, 250}
    assert {p.get("fallback", 0) for p in params} >= {0, 147}
    assert {p.get("max_insert_size", 1000) for p in params} >= {12, 30, 1000, 6000}
    results = {(r["file"], json.dumps(r["params"], sort_keys=True)): r["fragment_length"] for r in meta["fraglen"]}
    assert results[("se_sparse", "{}")] == 0 and results[("se_sparse", '{"fallback": 147}')] == 147
    assert results[("se_peaks", "{}")] != results[("se_peaks", '{"flag_exclude": 16}')]     # a flag_exclude that changes the outcome
    assert 120 <= results[("se_peaks", "{}")] <= 240 and 30 <= results[("se_dense", "{}")] <= 55  # real strand structure: a peak
    for key in ("paired", "readlen", "mapped", "metadata", "chrom_reads"):
        assert meta[key]


def test_early_exit_is_hit_in_each_place(gold, caches):
    """The exit inside the first contig, exactly at its end, and in the second one (what the statement went through)."""
    _, meta, files = gold
    seen = set()
    for early_exit in (1, 3, 4, 5, 250):
        details = {}
        expected.fragment_length(files["se_peaks"], details, caches["se_peaks"], max_iterations=3, early_exit=early_exit, lag_step=1)
        assert details["blocks"][0] == 3 and details["candidates"][0] == min(3, early_exit)
        seen.add((len(details["candidates"]), sum(details["candidates"]) >= early_exit))
    assert seen == {(1, True), (2, True), (3, False)}


def test_paired_templates_are_odd_and_even(gold, caches):
    """The median of the paired branch over an odd and over an even number of templates, below and at its cap."""
    _, meta, files = gold
    counts = {}
    for r in meta["fraglen"]:
        if r["file"] in ("pe_a", "pe_b", "pe_many", "mixed"):
            details = {}
            expected.fragment_length(files[r["file"]], details, caches[r["file"]], **r["params"])
            if details["sampled"] and details["paired"]:
                counts.setdefault(r["file"], set()).add(details["templates"])
    below_cap = {n for key in ("pe_a", "pe_b", "mixed") for n in counts[key] if n > 0}
    assert {n % 2 for n in below_cap} == {0, 1} and max(below_cap) < 2000
    assert 2000 in counts["pe_many"] and max(counts["pe_many"]) > 2000  # at the cap of 2 000, and above it with more iterations


def test_paired_end_probe_equals_the_reference(gold):
    _, meta, files = gold
    for r in meta["paired"]:
        assert int(expected.is_paired_end(files[r["file"]], r["max_reads"])) == r["paired"], r
    assert {(r["file"], r["max_reads"], r["paired"]) for r in meta["paired"]} >= {("mixed", 1000, 0), ("mixed", 0, 1), ("pe_a", 1, 1)}


def test_read_length_probe_equals_the_reference(gold):
    _, meta, files = gold
    outcomes = set()
    for r in meta["readlen"]:
        if r["error"] is not None:
            with pytest.raises(RuntimeError, match=r["error"]):
                expected.read_length(files[r["file"]], r["min_reads"], r["max_iterations"], r["flag_exclude"])
        else:
            assert expected.read_length(files[r["file"]], r["min_reads"], r["max_iterations"], r["flag_exclude"]) == r["read_length"], r
        if r["file"] == "se_peaks" and (r["min_reads"], r["max_iterations"]) == (32, 4096):
            outcomes.add((r["flag_exclude"], r["read_length"]))
    assert {(0, 75), (4, 36)} <= outcomes  # a flag_exclude that changes the outcome: unmapped records lead the file


def test_mapped_read_count_equals_the_reference(gold):
    _, meta, files = gold
    for r in meta["mapped"]:
        assert expected.mapped_read_count(files[r["file"]], tuple(r["exclude"])) == (r["mapped"], r["unmapped"]), r
    assert any(r["unmapped"] > 0 for r in meta["mapped"])


def test_fragment_length_equals_the_reference(gold, caches):
    _, meta, files = gold
    for r in meta["fraglen"]:
        assert expected.fragment_length(files[r["file"]], cache=caches[r["file"]], **r["params"]) == r["fragment_length"], r


def test_count_metadata_equals_the_reference(gold, caches):
    _, meta, files = gold
    levels = set()
    for r in meta["metadata"]:
        if r["error"] is not None:
            with pytest.raises(RuntimeError, match=r["error"]):
                expected.count_metadata(files[r["file"]], **r["call"])
            continue
        metadata, log = expected.count_metadata(files[r["file"]], cache=caches[r["file"]], **r["call"])
        assert metadata == r["metadata"] and log == r["log"], r
        levels.update(level for level, _ in log)
        levels.update(message.split(" ")[0] for _, message in log)
    assert levels >= {"INFO", "WARNING", "Using", "Could", "`extend_reads=0`"}  # each of the three log lines


def test_records_carry_an_optional_query_length():
    six = (np.array([1, 5]), np.array([51, 55]), np.array([0, 0]), np.array([0, 16]), np.array([30, 30]), np.array([0, 0]))
    plain = AlignmentRecords(*six)
    assert plain.qlen is None and len(plain) == 2
    with_length = AlignmentRecords.with_query_length(*six, np.array([50, 50]))
    assert with_length.qlen.dtype == np.int32 and with_length.qlen.tolist() == [50, 50]
    assert AlignmentRecords(*six, qlen=[50, 36]).qlen.tolist() == [50, 36]
    with pytest.raises(ValueError, match="qlen"):
        AlignmentRecords(*six, qlen=np.array([50]))
    with pytest.raises(TypeError, match="qlen"):
        AlignmentRecords(*six, qlen=np.array([50.0, 50.0]))
    assert rt._records_slice(with_length, 1, 2).qlen.tolist() == [50] and rt._records_slice(plain, 0, 1).qlen is None


def test_unchecked_constructor_round_trips_and_keeps_the_query_length():
    six = (np.array([1, 5, 9]), np.array([51, 55, 59]), np.array([0, 0, 0]), np.array([0, 16, 0]), np.array([30, 30, 0]), np.array([0, 0, 1]))
    checked = AlignmentRecords.with_query_length(*six, np.array([50, 36, 20]))
    names = ("pos", "end", "isize", "flag", "mapq", "mate_same", "qlen")
    made = AlignmentRecords._of(*[getattr(checked, name) for name in names])
    assert type(made) is AlignmentRecords and len(made) == 3 and all(getattr(made, name) is getattr(checked, name) for name in names)
    part = rt._records_slice(made, 1, 3)
    for name in names:
        got, want = getattr(part, name), getattr(checked, name)[1:3]
        assert got.dtype == want.dtype and got.tolist() == want.tolist(), name
    assert part.qlen.tolist() == [36, 20]
    assert AlignmentRecords._of(*[getattr(checked, name) for name in names[:6]]).qlen is None


def test_query_length_errors_word_for_word():
    six = (np.array([1, 5]), np.array([51, 55]), np.array([0, 0]), np.array([0, 16]), np.array([30, 30]), np.array([0, 0]))
    for bad, error, text in ((np.array([[50, 50]]), ValueError, "AlignmentRecords: `qlen` must be one-dimensional"),
                             (np.array([50.0, 50.0]), TypeError, "AlignmentRecords: `qlen` must hold integers, not float64"),
                             (np.array([50, 2 ** 31]), ValueError, "AlignmentRecords: `qlen` does not fit int32"),
                             (np.array([50, -2 ** 31 - 1]), ValueError, "AlignmentRecords: `qlen` does not fit int32"),
                             (np.array([50, 50, 50]), ValueError, "AlignmentRecords: `qlen` has 3 entries, `pos` has 2")):
        with pytest.raises(error) as info:
            AlignmentRecords(*six, qlen=bad)
        assert str(info.value) == text


def test_probes_name_a_missing_query_length():
    six = (np.array([1, 5]), np.array([51, 55]), np.array([0, 0]), np.array([0, 16]), np.array([30, 30]), np.array([0, 0]))
    file = AlignmentFileRecords([("chrA", 10000)], {"chrA": AlignmentRecords(*six)}, name="sample.bam")
    with pytest.raises(ValueError, match="qlen"):
        rt.alignment_read_length_from_records(file)
    with pytest.raises(ValueError, match="qlen"):
        rt.alignment_fragment_length_from_records(file)
    with pytest.raises(ValueError, match="header does not name"):
        AlignmentFileRecords([("chrA", 10000)], {"chrB": AlignmentRecords(*six)})


def test_head_probes_on_host_arrays_equal_the_reference(gold):
    """The two head-of-file probes are host arithmetic on a head slice: with NumPy records they run without a device."""
    _, meta, files = gold
    built = {key: AlignmentFileRecords(contigs, {n: AlignmentRecords(*[r[f] for f in expected.FIELDS[:6]], qlen=r["qlen"])
                                                  for n, r in records.items()}, name=key) for key, (contigs, records) in files.items()}
    for r in meta["paired"]:
        assert int(rt.is_alignment_paired_end_from_records(built[r["file"]], r["max_reads"])) == r["paired"], r
    for r in meta["readlen"]:
        if r["error"] is not None:
            with pytest.raises(RuntimeError, match=r["error"]):
                rt.alignment_read_length_from_records(built[r["file"]], r["min_reads"], r["max_iterations"], r["flag_exclude"])
        else:
            assert rt.alignment_read_length_from_records(built[r["file"]], r["min_reads"], r["max_iterations"],
                                                         r["flag_exclude"]) == r["read_length"], r
    for key, (contigs, _) in files.items():
        assert rt._top_contigs(contigs) == expected.top_contigs(contigs)
        top = [n for n, _ in expected.top_contigs(contigs)]
        for flag_exclude, max_iterations in [(0, 1000), (0, 1), (16, 3), (1024, 4096), (65535, 10)]:
            assert rt._sample_pass(built[key].tracks(top), flag_exclude, max_iterations) == \
                expected.sample_pass(files[key], expected.top_contigs(contigs), flag_exclude, max_iterations)
