"""Row f12 on the GPU: `rocco_amd.scores`' functions over BAM PATHS -- raw_count_matrix, get_read_length, get_ecdf,
multi_ecdf, score_peaks -- against what the reference's own functions wrote for the same files
(tests/golden/score_paths.*, made by tests/golden/make_golden_score_paths.py).  Every comparison is exact: integers,
file bytes, float64 bit patterns, log records.  Then the routes through the pass: one contig per group against one group,
one file per call against all, both inflate modes, files with and without their index."""
import os

import numpy as np
import pytest

import score_paths_files as sp

pytestmark = pytest.mark.gpu
ERRORS = {"IndexError": IndexError, "TypeError": TypeError, "ValueError": ValueError}


@pytest.fixture(scope="module")
def paths(gpu, tmp_path_factory):
    from rocco_amd import bam

    bam.clear_alignment_cache()
    yield sp.write_files(tmp_path_factory.mktemp("score_paths"))
    bam.clear_alignment_cache()


def bams(paths):
    return [paths[k] for k in sp.FILES]


def in_dir(paths, name):
    return os.path.join(paths["dir"], name)


def file_bytes(path):
    with open(path, "rb") as handle:
        return handle.read()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_score_case(paths, entry, label=None, **more):
    """score_peaks as the generator called the reference's: (result, log, narrowPeak bytes, TSV bytes)."""
    from rocco_amd import scores

    label = label or entry["name"]
    matrix, scored = in_dir(paths, f"{label}.counts.tsv"), in_dir(paths, f"{label}.narrowPeak")
    for stale in (matrix, scored):
        if os.path.exists(stale):
            os.remove(stale)
    if entry["existing_matrix"]:
        with open(matrix, "wb") as handle:
            handle.write(sp.golden()[0]["score_no_matrix_tsv"].tobytes())
    result, log = sp.logged(lambda: scores.score_peaks(bams(paths), chrom_sizes_file=paths["g.sizes"], peak_file=paths["peaks.bed"],
                                                       count_matrix_file=matrix, output_file=scored, threads=1, proc=1,
                                                       summit_offsets_file=paths["summits.tsv"], **entry["kwargs"], **more), paths["dir"])
    return result, log, file_bytes(scored), file_bytes(matrix)


def check_score_case(arrays, entry, result, log, narrowpeak, tsv, label=None):
    name = entry["name"]
    assert narrowpeak == arrays[f"score_{name}_narrowpeak"].tobytes() and tsv == arrays[f"score_{name}_tsv"].tobytes(), name
    assert same_bits(result[0], arrays[f"score_{name}_scores"]) and same_bits(result[2], arrays[f"score_{name}_pvals"]), name
    assert np.array_equal(np.asarray(result[1]), arrays[f"score_{name}_bed6"]), name
    if label is None:
        assert log == entry["log"], name


def test_read_lengths_mapped_counts_and_skip_counts(paths):
    from rocco_amd import bam
    from rocco_amd import scores

    arrays, meta = sp.golden()
    for entry in meta["read_length"]:
        call = lambda: scores.get_read_length(paths[entry["file"]], entry["num_reads"], entry["min_mapping_quality"])
        if entry["error"] is not None:
            with pytest.raises(ERRORS[entry["error"]], match=entry["file"] + ".bam"):
                call()
        else:
            value = call()
            assert type(value) is int and value == entry["value"], entry
    files = [bam._cached_file(p) for p in bams(paths)]
    assert scores._read_lengths(files) == [e["value"] for e in meta["read_length"] if e["file"] in sp.FILES and e["num_reads"] == 1000]
    for key, file in zip(sp.FILES, files):
        assert scores._mapped_reads(file) == meta["mapped"][key]
        for t, name in enumerate(sp.contig_names(key)):
            assert scores._contig_count(file, name) == arrays[f"itr_{key}_{t}"].size == meta["files"][key]["refs"][t]["records"]
        with pytest.raises(ValueError, match="invalid contig `chrQ`"):
            scores._contig_count(file, "chrQ")


def test_read_length_turns_fetch_all_short_files_in_one_call(paths, monkeypatch):
    """Per turn ONE `_load_contigs` call over the next non-empty contig of every file that is still short."""
    from rocco_amd import bam
    from rocco_amd import scores

    bam.clear_alignment_cache()
    files = [bam._cached_file(p) for p in bams(paths)]
    turns, load = [], bam._load_contigs
    monkeypatch.setattr(bam, "_load_contigs", lambda pairs: (turns.append([(os.path.basename(f.path), c) for f, c in pairs]), load(pairs))[1])
    scores._read_lengths(files)
    # p1 fills its 1000 inside chr1; p2 needs chr2, chrY and chrM as well; p3 runs out (it has no chrY records); chrX is never fetched
    assert turns == [[("p1.bam", "chr1"), ("p2.bam", "chr1"), ("p3.bam", "chr1")], [("p2.bam", "chr2"), ("p3.bam", "chr2")],
                     [("p2.bam", "chrY"), ("p3.bam", "chrM")], [("p2.bam", "chrM")]]


def test_raw_count_matrix_bytes_and_log(paths):
    from rocco_amd import scores

    arrays, meta = sp.golden()
    tsv = in_dir(paths, "raw.counts.tsv")
    if os.path.exists(tsv):
        os.remove(tsv)
    out, log = sp.logged(lambda: scores.raw_count_matrix(bams(paths), paths["peaks.bed"], tsv, bed_columns=3), paths["dir"])
    assert out == tsv and file_bytes(tsv) == arrays["raw_count_matrix_tsv"].tobytes() and log == meta["raw_count_matrix_log"]
    _, log = sp.logged(lambda: scores.raw_count_matrix(bams(paths), paths["peaks.bed"], tsv, bed_columns=3), paths["dir"])
    assert file_bytes(tsv) == arrays["raw_count_matrix_tsv"].tobytes() and log == meta["raw_count_matrix_again_log"]
    assert any(level == "WARNING" for level, _ in log)
    listing = in_dir(paths, "files.txt")  # a text file of paths (check_type_bam_files)
    with open(listing, "w") as handle:
        handle.write("\n".join(bams(paths)) + "\n")
    os.remove(tsv)
    scores.raw_count_matrix(listing, paths["peaks.bed"], tsv)
    assert file_bytes(tsv) == arrays["raw_count_matrix_tsv"].tobytes()


def test_get_ecdf_and_multi_ecdf_by_bit_pattern(paths):
    from rocco_amd import scores

    arrays, meta = sp.golden()
    for entry in meta["get_ecdf"]:
        null, log = sp.logged(lambda: scores.get_ecdf(bams(paths), chrom_sizes_file=paths["g.sizes"], **entry["kwargs"]), paths["dir"])
        assert same_bits(null.values, arrays[f"ecdf_{entry['name']}_values"]) and log == entry["log"], entry["name"]
    entry = meta["multi_ecdf"]
    nulls, log = sp.logged(lambda: scores.multi_ecdf(bams(paths), chrom_sizes_file=paths["g.sizes"], proc=1, **entry["kwargs"]), paths["dir"])
    assert [int(k) for k in nulls] == arrays["multi_ecdf_lengths"].tolist() and log == entry["log"]
    for length, null in nulls.items():
        assert same_bits(null.values, arrays[f"multi_ecdf_{int(length)}"]), length


@pytest.mark.parametrize("case", [0, 1, 2])
def test_score_peaks_files_arrays_and_log(paths, case):
    arrays, meta = sp.golden()
    entry = meta["score_peaks"][case]
    assert entry["error"] is None
    check_score_case(arrays, entry, *run_score_case(paths, entry))


def test_score_peaks_with_an_existing_matrix_counts_the_nulls_only(paths, monkeypatch):
    from rocco_amd import readtracks
    from rocco_amd import scores

    arrays, meta = sp.golden()
    seen, count = [], readtracks.count_alignment_intervals_sets_device
    monkeypatch.setattr(readtracks, "count_alignment_intervals_sets_device",
                        lambda files, chroms, starts, ends, sets, options, *a, **kw: (seen.append((sorted(set(np.asarray(sets).tolist())), list(options))),
                                                                                      count(files, chroms, starts, ends, sets, options, *a, **kw))[1])
    run_score_case(paths, meta["score_peaks"][1])
    assert seen == [([0], [scores.NULL_COUNT_OPTIONS])]
    del seen[:]
    run_score_case(paths, meta["score_peaks"][0])
    assert seen == [([0, 1], [scores.RAW_COUNT_OPTIONS, scores.NULL_COUNT_OPTIONS])]  # the peaks and the nulls of a group in ONE call


def test_a_skip_contig_the_header_does_not_have(paths):
    from rocco_amd import scores

    _, meta = sp.golden()
    entry = meta["skip_absent"]
    with pytest.raises(ERRORS[entry["error"]], match="invalid contig `chrM`"):
        scores.score_peaks([paths[entry["file"]]], chrom_sizes_file=paths["wide.sizes"], peak_file=paths["wide.bed"],
                           count_matrix_file=in_dir(paths, "wide.counts.tsv"), output_file=in_dir(paths, "wide.narrowPeak"),
                           skip_for_norm=entry["skip_for_norm"], ecdf_nsamples=5, seed=3, threads=1, proc=1)
    with pytest.raises(ValueError, match="chromosome not found in alignment header"):  # (as the *_from_records forms)
        scores.get_ecdf([paths["wide"]], 300, paths["g.sizes"], nsamples=20, seed=1)


def test_path_functions_equal_their_from_records_forms(paths):
    from rocco_amd import bam
    from rocco_amd import scores

    arrays, meta = sp.golden()
    files = [bam._cached_file(p) for p in bams(paths)]
    names = sp.contig_names("p1")
    records = [{c: file.records[c] for c in names} for file in files]
    tsv = in_dir(paths, "from_records.counts.tsv")
    scores.raw_count_matrix_from_records(records, sp.FILES, paths["peaks.bed"], tsv)
    assert file_bytes(tsv) == arrays["raw_count_matrix_tsv"].tobytes()
    kwargs = meta["get_ecdf"][1]["kwargs"]
    null = scores.get_ecdf_from_records(records, chrom_sizes_file=paths["g.sizes"], **kwargs)
    assert same_bits(null.values, scores.get_ecdf(bams(paths), chrom_sizes_file=paths["g.sizes"], **kwargs).values)
    entry = meta["score_peaks"][2]
    mapped, lengths = scores._norm_facts(files, entry["kwargs"]["skip_for_norm"])
    skipped = sum(r["records"] for r in meta["files"]["p1"]["refs"][3:4])
    assert mapped[0] == meta["mapped"]["p1"] - skipped and skipped > 0  # chrY has records
    os.remove(tsv)
    scored = in_dir(paths, "from_records.narrowPeak")
    result = scores.score_peaks_from_records(records, sp.FILES, paths["g.sizes"], paths["peaks.bed"], mapped, lengths, count_matrix_file=tsv,
                                             output_file=scored, summit_offsets_file=paths["summits.tsv"], **entry["kwargs"])
    check_score_case(arrays, entry, result, None, file_bytes(scored), file_bytes(tsv), label="from_records")


def counted(monkeypatch):
    """([_load_contigs calls], [counting calls]) of what runs next, counted as the f11 tests count launches."""
    from rocco_amd import bam
    from rocco_amd import readtracks

    loads, counts = [], []
    load, count = bam._load_contigs, readtracks.count_alignment_intervals_sets_device
    monkeypatch.setattr(bam, "_load_contigs", lambda pairs: (loads.append(sorted({c for _, c in pairs})), load(pairs))[1])
    monkeypatch.setattr(readtracks, "count_alignment_intervals_sets_device",
                        lambda files, *a, **kw: (counts.append((len(files), kw.get("col0", 0))), count(files, *a, **kw))[1])
    return loads, counts


def test_one_contig_per_group_against_one_group(paths, monkeypatch):
    """`GROUP_BYTES` below every contig: five groups (the peaks lie on all five contigs), each fetched with one
    `_load_contigs` call and counted with one call; the default budget: one group, one fetch, one call.  Same files."""
    from rocco_amd import bam
    from rocco_amd import scores

    arrays, meta = sp.golden()
    tsv = in_dir(paths, "groups.counts.tsv")
    loads, counts = counted(monkeypatch)
    for budget, groups in ((1, [["chr1"], ["chrX"], ["chr2"], ["chrY"], ["chrM"]]), (scores.GROUP_BYTES, [["chr1", "chr2", "chrM", "chrX", "chrY"]])):
        monkeypatch.setattr(scores, "GROUP_BYTES", budget)
        bam.clear_alignment_cache()
        del loads[:], counts[:]
        scores.raw_count_matrix(bams(paths), paths["peaks.bed"], tsv)
        assert loads == groups and counts == [(3, 0)] * len(groups), budget
        assert file_bytes(tsv) == arrays["raw_count_matrix_tsv"].tobytes()
    # contigs without intervals are never decoded: regions of 60 kb fit chr2 only
    bam.clear_alignment_cache()
    del loads[:], counts[:]
    scores.get_ecdf(bams(paths), 60000, paths["g.sizes"], nsamples=10, seed=2)
    assert loads == [["chr2"]] and counts == [(3, 0)]
    # score_peaks, one contig per group: the bytes of the one-group run (the test above)
    monkeypatch.setattr(scores, "GROUP_BYTES", 1)
    bam.clear_alignment_cache()
    del loads[:], counts[:]
    entry = meta["score_peaks"][0]
    check_score_case(arrays, entry, *run_score_case(paths, entry, label="grouped"), label="grouped")
    assert counts == [(3, 0)] * 5 and loads[:5] == [["chr1"], ["chrX"], ["chr2"], ["chrY"], ["chrM"]]  # (then the read-length turns)


def test_one_file_per_call_against_all_files(paths, monkeypatch):
    arrays, meta = sp.golden()
    loads, counts = counted(monkeypatch)
    entry = meta["score_peaks"][0]
    check_score_case(arrays, entry, *run_score_case(paths, entry, label="columns", files_per_call=1), label="columns")
    assert counts == [(1, 0), (1, 1), (1, 2)]
    del counts[:]
    check_score_case(arrays, entry, *run_score_case(paths, entry, label="columns", files_per_call=2), label="columns")
    assert counts == [(2, 0), (1, 2)]
    from rocco_amd import scores

    with pytest.raises(ValueError, match="files_per_call"):
        scores.raw_count_matrix(bams(paths), paths["peaks.bed"], in_dir(paths, "never.tsv"), files_per_call=0)


@pytest.mark.parametrize("route", ["device_inflate", "no_bai", "use_index_off", "mixed"])
def test_every_route_to_the_records_gives_the_same_files(gpu, tmp_path, monkeypatch, route):
    """Both inflate modes; files without their `.bai`; `USE_INDEX` off; one file of three without an index (the resident
    whole-file route and the indexed route through the same counting call)."""
    from rocco_amd import bam
    from rocco_amd import scores

    arrays, meta = sp.golden()
    local = sp.write_files(tmp_path, with_index=route != "no_bai")
    if route == "device_inflate":
        monkeypatch.setattr(bam, "DEFAULT_INFLATE", "device")
    if route == "use_index_off":
        monkeypatch.setattr(bam, "USE_INDEX", False)
    if route == "mixed":
        os.remove(local["p2"] + ".bai")
    bam.clear_alignment_cache()
    try:
        files = [bam._cached_file(local[k]) for k in sp.FILES]
        indexed = [isinstance(f, bam.IndexedAlignmentFile) for f in files]
        assert indexed == {"device_inflate": [True] * 3, "no_bai": [False] * 3, "use_index_off": [False] * 3, "mixed": [True, False, True]}[route]
        entry = meta["score_peaks"][2]
        check_score_case(arrays, entry, *run_score_case(local, entry))
        for e in meta["read_length"]:
            if e["file"] in sp.FILES:
                assert scores.get_read_length(local[e["file"]], e["num_reads"], e["min_mapping_quality"]) == e["value"], (route, e)
        assert [scores._mapped_reads(f) for f in files] == [meta["mapped"][k] for k in sp.FILES]
    finally:
        bam.clear_alignment_cache()


def test_a_track_out_of_coordinate_order_is_refused(gpu, tmp_path):
    """What the *_from_records forms raise today, through the path functions (a resident file whose chr1 records are swapped)."""
    import torch

    from rocco_amd import bam
    from rocco_amd import scores

    local = sp.write_files(tmp_path, with_index=False)
    bam.clear_alignment_cache()
    try:
        file = bam._cached_file(local["p2"])
        pos = file.records["chr1"].pos
        a, b = int(pos[100]), int(pos[300])
        assert a < b
        pos[100], pos[300] = b, a
        with pytest.raises(ValueError, match="file 1 on chr1 are not in coordinate order"):
            scores.raw_count_matrix([local[k] for k in sp.FILES], local["peaks.bed"], os.path.join(local["dir"], "never.tsv"))
        torch.cuda.synchronize()
    finally:
        bam.clear_alignment_cache()
