"""GPU: a BAM path through rocco_amd.bam's entry points with the reference's signatures against
what the REFERENCE's own get_bam_chrom_reads, _get_bam_count_metadata and generate_chrom_matrix returned for the same files
(tests/golden/bam_files.npz, written by tests/golden/make_golden_bam_files.py over htslib and the reference's compiled
counter): arrays by their bytes, log lines and errors word for word."""
import logging
import multiprocessing
import os

import numpy as np
import pytest

import bam_expected as bx

pytestmark = pytest.mark.gpu

READER_FILES = ["mixed", "blocks", "longread", "one_record", "header_only", "decoy"]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    from rocco_amd import bam

    root = tmp_path_factory.mktemp("bam_files")
    _, meta = bx.golden()
    out = {key: bx.write_bam(root, key) for key in READER_FILES}
    out["sizes"] = str(root / "t.sizes")
    with open(out["sizes"], "w") as handle:
        handle.write("".join(f"{name}\t{length}\n" for name, length in meta["sizes"]))
    bam.clear_alignment_cache()
    yield out
    bam.clear_alignment_cache()


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def logged(call, paths):
    from rocco_amd import bam

    keep = Keep()
    bam.logger.addHandler(keep)
    level = bam.logger.level
    bam.logger.setLevel(logging.DEBUG)
    bam._BAM_COUNT_METADATA_CACHE.clear()
    try:
        result = call()
    finally:
        bam.logger.removeHandler(keep)
        bam.logger.setLevel(level)
    log = []
    for level_name, message in keep.records:
        for key, path in paths.items():
            message = message.replace(path, "{" + key + "}")
        log.append([level_name, message])
    return result, log


@pytest.mark.parametrize("key", READER_FILES)
def test_get_bam_chrom_reads_as_the_reference_ran_it(gpu, paths, key):
    """Every contig of the file (and one the header does not name) under the four option sets of the fixture script: the
    reference's (intervals, values) by their bytes, its (None, None) returns with their warnings, its errors."""
    from rocco_amd import bam

    arrays, meta = bx.golden()
    seen = 0
    for entry in meta["chrom_reads"]:
        if entry["file"] != key:
            continue
        seen += 1
        name = entry["name"]
        call = lambda: bam.get_bam_chrom_reads(paths[key], entry["contig"], paths["sizes"], entry["step"], **entry["kwargs"])
        if entry["error"] is not None:
            with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[entry["error_type"]]) as info:
                call()
            assert str(info.value).replace(paths["sizes"], "{sizes}") == entry["error"], name
            continue
        (intervals, vals), log = logged(call, paths)
        assert log == entry["log"], name
        if entry["none"]:
            assert intervals is None and vals is None, name
            continue
        want_i, want_v = arrays[f"r_{name}_intervals"], arrays[f"r_{name}_values"]
        assert intervals.dtype == want_i.dtype and np.array_equal(intervals, want_i), name
        assert vals.dtype == want_v.dtype and vals.tobytes() == want_v.tobytes(), name
    assert seen == 16


def test_reader_errors_are_the_references(gpu, paths, tmp_path):
    from rocco_amd import bam

    _, meta = bx.golden()
    calls = {"missing_bam": lambda: bam.get_bam_chrom_reads(str(tmp_path / "none.bam"), "chrA", paths["sizes"], 50),
             "missing_sizes": lambda: bam.get_bam_chrom_reads(paths["mixed"], "chrA", str(tmp_path / "none.sizes"), 50),
             "missing_chromosome": lambda: bam.get_bam_chrom_reads(paths["mixed"], "chrQ", paths["sizes"], 50)}
    assert sorted(e["label"] for e in meta["errors"]) == sorted(calls)
    for entry in meta["errors"]:
        with pytest.raises({"FileNotFoundError": FileNotFoundError, "ValueError": ValueError}[entry["type"]]) as info:
            calls[entry["label"]]()
        text = str(info.value).replace(str(tmp_path / "none.bam"), "{bam}").replace(str(tmp_path / "none.sizes"), "{sizes}")
        assert text.replace(paths["sizes"], "{sizes}") == entry["message"]


def test_get_bam_count_metadata_as_the_reference_ran_it(gpu, paths):
    """The reference's dict (its `threads` key by its own rule), its log lines, and its cache key: a second call with an
    equal key returns the cached dict without a log line."""
    from rocco_amd import bam

    _, meta = bx.golden()
    assert len(meta["metadata"]) == 8
    for entry in meta["metadata"]:
        call = lambda: bam._get_bam_count_metadata(paths[entry["file"]], **entry["call"])
        metadata, log = logged(call, paths)
        assert metadata == entry["metadata"] and log == entry["log"], entry
        assert {k: type(v) for k, v in metadata.items()} == {k: type(v) for k, v in entry["metadata"].items()}
        keep = Keep()
        bam.logger.addHandler(keep)
        try:
            assert call() is metadata and keep.records == []
        finally:
            bam.logger.removeHandler(keep)
    unresolved = bam._get_bam_count_metadata(paths["mixed"], 50, "CPM", -1, None, num_processors=-1)
    assert unresolved["threads"] == max(multiprocessing.cpu_count() - 1, 1)
    key = (paths["mixed"], 50, "CPM", -1.0, (), 0, -1, unresolved["threads"], 1.0)
    assert bam._BAM_COUNT_METADATA_CACHE[key] is unresolved


def test_generate_chrom_matrix_over_three_bam_files(gpu, paths, monkeypatch):
    """rocco_amd.readtracks.generate_chrom_matrix with the reader bound as INTEGRATION.md says, against the matrix the
    reference's own function produced; every file is decoded once and then served from the cache."""
    from rocco_amd import bam, readtracks

    arrays, meta = bx.golden()
    monkeypatch.setattr(readtracks, "get_bam_chrom_reads", bam.get_bam_chrom_reads)
    bam.clear_alignment_cache()
    decoded = []
    read = bam.read_alignment_file
    monkeypatch.setattr(bam, "read_alignment_file", lambda path, *a, **kw: (decoded.append(path), read(path, *a, **kw))[1])
    for record in meta["matrix"]:
        files = [paths[k] for k in record["files"]]
        intervals, matrix = readtracks.generate_chrom_matrix(record["contig"], files, paths["sizes"], record["step"], **record["kwargs"])
        want_i, want_m = arrays[f"{record['name']}_intervals"], arrays[f"{record['name']}_matrix"]
        assert intervals.dtype == want_i.dtype and np.array_equal(intervals, want_i), record["name"]
        assert matrix.dtype == want_m.dtype and matrix.shape == want_m.shape and matrix.tobytes() == want_m.tobytes(), record["name"]
    assert sorted(decoded) == sorted(paths[k] for k in meta["matrix"][0]["files"])
    assert len(bam._ALIGNMENT_CACHE) == 3
    # a file that changes on disk is decoded again; the byte budget drops the least recently used
    os.utime(paths["mixed"], ns=(1, 1))
    bam.get_bam_chrom_reads(paths["mixed"], "chrA", paths["sizes"], 50, effective_genome_size=2.7e9)
    assert decoded.count(paths["mixed"]) == 2
    monkeypatch.setattr(bam, "ALIGNMENT_CACHE_BYTES", 1)
    bam.get_bam_chrom_reads(paths["one_record"], "chrA", paths["sizes"], 50, effective_genome_size=2.7e9)
    assert len(bam._ALIGNMENT_CACHE) == 1
    bam.clear_alignment_cache()
    assert len(bam._ALIGNMENT_CACHE) == 0 and len(bam._BAM_COUNT_METADATA_CACHE) == 0
