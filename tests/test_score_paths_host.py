"""Row f12 without a GPU: the host rules of the scoring over BAM paths -- the read-length rule as a function of (flag,
mapq, qlen), the contig grouping under a byte budget, the sidecar naming of the narrowPeak step, `check_type_bam_files` --
against what the reference wrote (tests/golden/score_paths.*), and the census the fixture files were made for."""
import ctypes
import os
import re

import numpy as np
import pytest

import score_paths_files as sp

ERRORS = {"IndexError": IndexError, "TypeError": TypeError, "ValueError": ValueError}


def test_read_length_rule_against_the_references_values():
    from rocco_amd.scores import read_length_from_fields

    _, meta = sp.golden()
    assert len(meta["read_length"]) == 18
    for entry in meta["read_length"]:
        rows = sp.fetch_rows(entry["file"])
        call = lambda: read_length_from_fields(rows[:, 4], rows[:, 5], rows[:, 7], entry["num_reads"], entry["min_mapping_quality"],
                                               name=entry["file"] + ".bam")
        if entry["error"] is not None:
            with pytest.raises(ERRORS[entry["error"]], match=re.escape(entry["file"] + ".bam")):
                call()
        else:
            value = call()
            assert type(value) is int and value == entry["value"], entry


def test_read_length_rule_on_chosen_records():
    from rocco_amd.scores import read_length_from_fields

    flag = np.array([0, 4, 256, 2048, 16, 0, 1 | 2 | 64, 0], dtype=np.uint16)
    mapq = np.array([10, 60, 60, 60, 9, 255, 30, 11], dtype=np.uint8)
    qlen = np.array([40, 1000, 1000, 1000, 1000, 60, 80, 100], dtype=np.int32)
    assert read_length_from_fields(flag, mapq, qlen) == int(np.percentile([40, 60, 80, 100], 75))
    assert read_length_from_fields(flag, mapq, qlen, num_reads=2) == int(np.percentile([40, 60], 75))
    assert read_length_from_fields(flag, mapq, qlen, num_reads=0) == 40  # (the reference appends before it tests the quota)
    assert read_length_from_fields(flag, mapq, qlen, min_mapping_quality=31) == 60
    # infer_query_length() is None for a query length of 0: np.percentile refuses the list, and so does the rule
    with pytest.raises(TypeError) as reference:
        int(np.percentile([40, None, 80], 75))
    with pytest.raises(type(reference.value), match="sample.bam"):
        read_length_from_fields(flag, mapq, np.where(qlen == 60, 0, qlen), name="sample.bam")
    assert read_length_from_fields(flag, mapq, np.where(qlen == 1000, 0, qlen)) == 85  # (a rejected record's length is never read)
    with pytest.raises(Exception) as reference:
        int(np.percentile([], 75))
    with pytest.raises(type(reference.value), match="sample.bam"):
        read_length_from_fields(flag, mapq, qlen, min_mapping_quality=256, name="sample.bam")


def test_census_of_the_fixture_files():
    arrays, meta = sp.golden()
    q = {}
    for key in sp.FILES:
        rows = sp.fetch_rows(key)
        table = arrays[f"rec_{key}"]
        assert rows.shape[0] == np.count_nonzero(table[:, 0] >= 0) and np.count_nonzero(table[:, 0] < 0) > 0  # an unplaced tail
        assert np.all(np.diff(rows[:, 0]) >= 0) and all(np.all(np.diff(rows[rows[:, 0] == t, 1]) >= 0) for t in range(5))
        assert np.all(table[(table[:, 4] & 4) == 0, 7] > 0), "a mapped record without a CIGAR"
        assert np.count_nonzero(rows[:, 0] == 1) == 0 and set(np.unique(rows[:, 0])) >= {0, 2, 4}  # chrX has no records
        assert rows[:, 5].min() == 0 and rows[:, 5].max() == 60
        assert all(np.count_nonzero(rows[:, 4] & bit) > 0 for bit in (1, 4, 256, 2048))
        keep = ((rows[:, 4] & (4 | 256 | 2048)) == 0) & (rows[:, 5] >= 10)
        q[key] = (rows, keep, np.cumsum(keep))
        assert meta["mapped"][key] == sum(r["mapped"] for r in meta["files"][key]["refs"]) == np.count_nonzero((rows[:, 4] & 4) == 0)
    assert [arrays[f"rec_{k}"].shape[0] for k in sp.FILES] == [meta["files"][k]["records"] for k in sp.FILES]
    assert 2500 < arrays["rec_p1"].shape[0] < 3500 and 1000 < arrays["rec_p2"].shape[0] < 1500 and 300 < arrays["rec_p3"].shape[0] < 500
    pile = arrays["rec_p1"]
    assert np.count_nonzero((pile[:, 0] == 2) & (pile[:, 1] == meta["pile_position"])) >= 600

    def contig_of_nth(key, n):
        rows, _, running = q[key]
        return int(rows[int(np.searchsorted(running, n)), 0]) if running[-1] >= n else None

    # num_reads = 1000: filled inside the first contig, across a contig boundary, never
    assert contig_of_nth("p1", 1000) == 0 and contig_of_nth("p2", 1000) not in (0, None) and contig_of_nth("p3", 1000) is None
    for key in sp.FILES:  # num_reads = 50: the cut falls inside a contig
        rows, keep, running = q[key]
        cut = int(np.searchsorted(running, 50))
        assert rows[cut, 0] == rows[cut + 1, 0] == 0
    rows, keep, running = q["p3"]  # one window holds a record that each of the four filters rejects
    window = rows[: int(np.searchsorted(running, 50)) + 1]
    assert all(np.count_nonzero(window[:, 4] & bit) > 0 for bit in (4, 256, 2048)) and np.count_nonzero(window[:, 5] < 10) > 0
    largest = max(os.path.getsize(os.path.join(sp.HERE, "golden", f)) for f in os.listdir(os.path.join(sp.HERE, "golden")))
    assert all(arrays[f"bam_{k}"].size <= largest for k in sp.FILES)


def test_contig_groups_under_a_byte_budget():
    from rocco_amd import bam
    from rocco_amd import scores

    assert scores.GROUP_BYTES == bam.ALIGNMENT_CACHE_BYTES // 2
    groups = scores._contig_groups
    names = list("abcdefg")
    assert groups(names, [4, 4, 4, 4, 4, 4, 4], 8) == [["a", "b"], ["c", "d"], ["e", "f"], ["g"]]
    assert groups(names, [4, 4, 4, 4, 4, 4, 4], 100) == [names]
    assert groups(names, [4, 4, 4, 4, 4, 4, 4], 1) == [[n] for n in names]          # every contig above the budget: alone
    assert groups(names, [1, 1, 50, 1, 1, 0, 6], 8) == [["a", "b"], ["c"], ["d", "e", "f", "g"]]  # a single contig above it
    assert groups(names, [1, None, 1, 1, None, None, 1], 8) == [["a"], ["b"], ["c", "d"], ["e"], ["f"], ["g"]]  # no statistics
    assert groups(names, [8, 0, 0, 1, 7, 1, 0], 8) == [["a", "b", "c"], ["d", "e"], ["f", "g"]]
    assert groups([], [], 8) == []
    rng = np.random.default_rng(3)
    for _ in range(200):
        costs = [None if rng.random() < 0.1 else int(c) for c in rng.integers(0, 30, size=12)]
        budget = int(rng.integers(1, 60))
        got = groups(list(range(12)), costs, budget)
        assert [c for g in got for c in g] == list(range(12))
        for g in got:
            assert len(g) == 1 or (all(costs[c] is not None for c in g) and sum(costs[c] for c in g) <= budget)
        for a, b in zip(got, got[1:]):  # greedy: the next contig did not fit
            assert any(costs[c] is None or costs[c] > budget for c in (a[-1], b[0])) or sum(costs[c] for c in a) + costs[b[0]] > budget


def test_sidecar_naming():
    from rocco_amd.rocco import narrowpeak_sidecar_root as root

    assert root("out/peaks.bed") == "out/peaks" and root("peaks.BED") == "peaks" and root("peaks.Bed") == "peaks"
    assert root("peaks") == "peaks" and root("peaks.txt") == "peaks.txt" and root("peaks.bed.gz") == "peaks.bed.gz"
    assert root("a.b/peaks") == "a.b/peaks" and root("peaks.narrowPeak") == "peaks.narrowPeak" and root(".bed") == ".bed"
    _, meta = sp.golden()
    for entry in meta["narrowpeak"]:  # the names the reference's step wrote
        if entry["files"]:
            assert sorted(os.path.basename(root(entry["output"])) + s for s in (".counts.tsv", ".narrowPeak")) == entry["files"]


def test_check_type_bam_files_errors(tmp_path):
    from rocco_amd.readtracks import check_type_bam_files

    a, b = tmp_path / "a.bam", tmp_path / "b.bam"
    a.write_bytes(b"")
    b.write_bytes(b"")
    listing = tmp_path / "files.txt"
    listing.write_text(f"{a}\n\n  {b}  \n")
    assert check_type_bam_files(str(listing)) == [str(a), str(b)]
    given = [str(b), str(a)]
    assert check_type_bam_files(given) is given
    listing.write_text(f"{a}\n{tmp_path}/gone.bam\n")
    with pytest.raises(FileNotFoundError) as info:
        check_type_bam_files(str(listing))
    assert str(info.value) == f"File in `bam_files_` not found: {tmp_path}/gone.bam"
    with pytest.raises(FileNotFoundError) as info:
        check_type_bam_files([str(a), f"{tmp_path}/gone.bam"])
    assert str(info.value) == f"File in `bam_files` not found: {tmp_path}/gone.bam"
    for bad in ((str(a),), None, 3):
        with pytest.raises(ValueError) as info:
            check_type_bam_files(bad)
        assert str(info.value) == "`bam_files` must be either a list or a path to a text file containing a list of BAM file paths."
    _, meta = sp.golden()  # the reference's own words for the missing file, as its narrowPeak step logged them
    failing = [e for e in meta["narrowpeak"] if e["missing_input"]][0]
    assert failing["log"][-1][1] == "\nCould not generate narrowPeak-formatted output\nFile in `bam_files` not found: {dir}/missing.bam"


def test_the_sets_entry_point_is_declared_and_bound():
    from rocco_amd import _native
    from rocco_amd import readtracks

    with open(os.path.join(os.path.dirname(sp.HERE), "include", "rocco_hip.h"), encoding="utf-8") as handle:
        text = handle.read()
    assert int(re.search(r"#define ROCCO_COUNT_INTERVALS_MAX_SETS (\d+)", text).group(1)) == readtracks.COUNT_INTERVALS_MAX_SETS == 4
    declared = re.search(r"^int rocco_hip_count_alignment_intervals_sets\(([^;]*)\);", text, re.M | re.S)
    params = [re.sub(r"\s+", " ", p).strip() for p in declared.group(1).split(",")]
    bound = {p[0]: p for p in _native.PROTOTYPES}["rocco_hip_count_alignment_intervals_sets"]
    assert bound[1] is ctypes.c_int and len(bound[2]) == len(params) == 24
    for param, argtype in zip(params, bound[2]):
        if param.endswith("_dev") or param in ("rocco_hip_solver *solver", "void *stream", "const rocco_hip_count_options *options_host"):
            assert argtype is ctypes.c_void_p, param
        elif param.startswith("size_t "):
            assert argtype is ctypes.c_size_t, param
        else:
            assert param in ("const int64_t *rec_offsets_host", "int32_t *track_facts_out_host") and argtype._type_ in (ctypes.c_longlong, ctypes.c_int)
    assert hasattr(_native.load(), "rocco_hip_count_alignment_intervals_sets")
