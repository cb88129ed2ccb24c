#!/usr/bin/env python3
"""What the REFERENCE's generate_chrom_matrix returns over BAM files, for the one-pass matrix of DESIGN.md section 0 row f9.

    python tests/golden/make_golden_bam_matrix.py        (by hand, where the reference is mounted; about a minute)

Every stored expectation was written by the reference's own ``generate_chrom_matrix`` (rocco/readtracks.py:521-633):

1. The reference's vendored htslib and the three drivers are built in a temporary directory exactly as
   make_golden_bam_files.py builds them (settings from the reference's own setup.py); nothing built or copied there is kept.
2. The BAM files are the bytes of tests/golden/bam_files.npz (indexed again by htslib) and four new small ones made here from
   SAM texts: `third_lo` / `third_hi`, whose reads lie in far-apart thirds of chrA (the union of their starts has a gap),
   and `touch_a` / `touch_b`, whose supports touch (last start + step == first start).  Both properties are asserted on
   what the reference returned.
3. ``generate_chrom_matrix`` runs with ``_require_native_counter`` replaced IN THE MODULE by a stand-in whose methods call
   the drivers; its return value, its error or its ``(None, None)`` and every log record of the call are kept.

Writes tests/golden/bam_matrix.npz + .json (data only: the new files' bytes, the expected arrays, the log records)."""
import ast
import importlib
import json
import logging
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bam_expected as bx  # noqa: E402

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="bam_matrix_")

# ---- 1. htslib and the drivers ---------------------------------------------------------------------------------------
HTS = os.path.join(WORK, "htslib")
shutil.copytree(os.path.join(REFERENCE, "vendor", "htslib"), HTS)


def reference_build_settings():
    """The module-level assignments and functions of the reference's setup.py (importing it would run ``setup()``)."""
    path = os.path.join(REFERENCE, "setup.py")
    with open(path, encoding="utf-8") as handle:
        tree = ast.parse(handle.read(), path)
    scope = {"__file__": path, "__name__": "reference_setup"}
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom, ast.Assign, ast.AnnAssign, ast.FunctionDef)):
            try:
                exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
            except NameError:
                pass
    return scope


SETTINGS = reference_build_settings()
for written, text in (("config.mk", SETTINGS["get_vendored_htslib_config_mk"]()), ("config.h", SETTINGS["get_vendored_htslib_config_h"]())):
    with open(os.path.join(HTS, written), "w", encoding="utf-8") as handle:
        handle.write(text)
SETTINGS["HTSCODECS_CONFIGURE_AC_PATH"] = os.path.join(HTS, "htscodecs", "configure.ac")
with open(os.path.join(HTS, "htscodecs", "htscodecs", "version.h"), "w", encoding="utf-8") as handle:
    handle.write(SETTINGS["get_vendored_htscodecs_version_h"]())
subprocess.run(["make", "-C", HTS, "-j16", "lib-static"], check=True, stdout=subprocess.DEVNULL)
BINARIES = {}
for binary, source, with_counter in (("files", "bam_files_driver.c", False), ("probe", "fragment_length_driver.c", True),
                                     ("count", "alignment_counts_driver.c", True)):
    BINARIES[binary] = os.path.join(WORK, binary)
    counter = [os.path.join(REFERENCE, "rocco", "native", "ccounts_backend.c")] if with_counter else []
    subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS, "-I", os.path.join(REFERENCE, "rocco", "native"),
                    os.path.join(HERE, source), *counter, os.path.join(HTS, "libhts.a"), "-lz", "-lm", "-lpthread", "-o", BINARIES[binary]],
                   check=True)


def driver(*args, binary="files"):
    return subprocess.run([BINARIES[binary], *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout


# ---- 2. the files ------------------------------------------------------------------------------------------------------
_, OLD_META = bx.golden()
CONTIGS = [(name, length) for name, length in OLD_META["sizes"] if name != "chrZ"]  # header order, as make_golden_bam_files.py wrote it
OLD_FILES = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only"]
BAMS, arrays = {}, {}
meta = {"sizes": OLD_META["sizes"], "old_files": OLD_FILES, "new_files": [], "scenarios": []}
for key in OLD_FILES:
    BAMS[key] = bx.write_bam(WORK, key)
    driver("index", BAMS[key])

rng = np.random.default_rng(20261)


def plain_reads(prefix, positions):
    """Single-end 50M reads on chrA at the 0-based ``positions``: either strand, mapping quality 20 .. 60, no sequence."""
    lines = []
    for i, pos0 in enumerate(positions):
        flag = 16 if rng.random() < 0.5 else 0
        lines.append(f"{prefix}{i}\t{flag}\tchrA\t{int(pos0) + 1}\t{int(rng.integers(20, 61))}\t50M\t*\t0\t0\t*\t*")
    return lines


def make_file(key, lines):
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in CONTIGS:
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for line in lines:
            handle.write(line + "\n")
    driver("sam2bam", sam, bam)
    driver("index", bam)
    BAMS[key] = bam
    with open(bam, "rb") as handle:
        arrays[f"bam_{key}"] = np.frombuffer(handle.read(), dtype=np.uint8)
    meta["new_files"].append(key)


make_file("third_lo", plain_reads("lo", np.sort(rng.integers(2000, 120000, size=300))))
make_file("third_hi", plain_reads("hi", np.sort(rng.integers(270000, 399000, size=300))))
make_file("touch_a", plain_reads("ta", 10000 + 50 * np.arange(100)))  # bins 10000 .. 14950 at step 50
make_file("touch_b", plain_reads("tb", 15000 + 50 * np.arange(100)))  # bins 15000 .. 19950

# ---- 3. the reference's own generate_chrom_matrix over a stand-in native module ------------------------------------------
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco")]
sys.modules["rocco"] = pkg
rt = importlib.import_module("rocco.readtracks")


class Native:
    """The compiled counter's methods (rocco/_hts_counts.c: names, keywords and defaults), answered by the drivers."""

    def is_alignment_paired_end(self, bam, max_reads=1000, thread_count=0):
        return bool(int(driver("paired", bam, max_reads, binary="probe")))

    def get_alignment_read_length(self, bam, min_reads=32, thread_count=0, max_iterations=4096, flag_exclude=0):
        text = driver("readlen", bam, min_reads, max_iterations, flag_exclude, binary="probe").strip()
        if text.startswith("ERROR "):
            raise RuntimeError(text[6:])
        return int(text)

    def get_alignment_mapped_read_count(self, bam, exclude_chromosomes=(), thread_count=0, count_mode="coverage", one_read_per_bin=0):
        mapped, unmapped = driver("mapped", bam, *exclude_chromosomes, binary="probe").split()
        return int(mapped), int(unmapped)

    def get_alignment_fragment_length(self, bam, thread_count=0, flag_exclude=0, max_iterations=1000, max_insert_size=1000,
                                      block_size=5000, rolling_chunk_size=250, lag_step=5, early_exit=250, fallback=0):
        return int(driver("fraglen", bam, flag_exclude, max_iterations, max_insert_size, block_size, rolling_chunk_size, lag_step,
                          early_exit, fallback, binary="probe"))

    def get_alignment_chrom_range(self, bam, chromosome, chrom_size, thread_count=1, flag_exclude=0):
        done = subprocess.run([BINARIES["count"], "range", bam, chromosome, str(chrom_size), str(flag_exclude)], capture_output=True, text=True)
        if done.returncode != 0:
            raise RuntimeError(done.stderr.strip().split(": ", 1)[-1])
        a, b = done.stdout.split()
        return int(a), int(b)

    def count_alignment_region(self, bam, chromosome, start, end, step, read_length, thread_count=1, count_mode="coverage",
                               one_read_per_bin=0, flag_include=0, flag_exclude=0, shift_forward_strand53=0, shift_reverse_strand53=0,
                               extend_bp=0, max_insert_size=1000, paired_end_mode=0, min_mapping_quality=0, min_template_length=-1,
                               **_ignored):
        assert count_mode == "coverage"
        out = os.path.join(WORK, "counts.f32")
        driver("count", bam, chromosome, start, end, step, ((end - start - 1) // step) + 1, 0, out, one_read_per_bin, flag_include,
               flag_exclude, shift_forward_strand53, shift_reverse_strand53, read_length, extend_bp, min_mapping_quality,
               min_template_length, max_insert_size, paired_end_mode, binary="count")
        return np.fromfile(out, dtype=np.float32)


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


rt._require_native_counter = lambda: Native()
rt.logger.setLevel(logging.DEBUG)
SIZES = os.path.join(WORK, "t.sizes")
with open(SIZES, "w") as handle:
    for name, length in meta["sizes"]:
        handle.write(f"{name}\t{length}\n")


def logged(call):
    keep = Keep()
    rt.logger.addHandler(keep)
    rt._BAM_COUNT_METADATA_CACHE.clear()
    try:
        result = call()
    finally:
        rt.logger.removeHandler(keep)
        log = []
        for level, message in keep.records:
            for key, bam in BAMS.items():
                message = message.replace(bam, "{" + key + "}")
            log.append([level, message.replace(SIZES, "{sizes}")])
        logged.last = log
    return result, log


RPGC = dict(effective_genome_size=2.7e9, num_processors=1)
CPM = dict(norm_method="CPM", num_processors=1)
ONE_SET = dict(norm_method="CPM", num_processors=1)  # the option set run on all three contigs (the binding test's input)
SCENARIOS = [
    ("gap", ["third_lo", "third_hi"], "chrA", 50, RPGC),
    ("touch", ["touch_a", "touch_b"], "chrA", 50, RPGC),
    ("small_files", ["mixed", "header_only", "one_record", "unplaced_only"], "chrA", 50, RPGC),
    ("one_record_kept", ["one_record", "mixed", "one_record"], "chrA", 50, RPGC),
    ("no_reads_excluded", ["mixed", "one_record", "blocks", "longread"], "chrC", 100, CPM),
    ("no_values_excluded", ["mixed", "one_record", "longread"], "chrA", 100, dict(norm_method="RPKM", flag_include=16, num_processors=1)),
    ("not_in_header", ["mixed", "blocks"], "chrZ", 50, CPM),
    ("all_excluded", ["blocks", "one_record"], "chrC", 50, CPM),
    ("single_file", ["longread"], "chrA", 50, RPGC),
    ("center_reads", ["mixed", "blocks"], "chrB", 50, dict(CPM, center_reads=True)),
    ("scale_by_step", ["mixed", "blocks", "longread"], "chrA", 200, dict(CPM, scale_by_step=True, const_scale=2.0)),
    ("round_digits", ["mixed", "blocks"], "chrB", 100, dict(norm_method="RPKM", round_digits=3, num_processors=1)),
    ("low_memory", ["third_lo", "mixed", "third_hi"], "chrA", 50, dict(RPGC, low_memory=True)),
    ("unplaced_file", ["mixed", "one_record", "unplaced_only"], "chrA", 50, RPGC),
    # float32 rows of an odd length start off a 16-byte boundary: the first of these steps at which m is odd is kept
    *[(f"low_memory_odd_{step}", ["third_hi", "touch_a", "third_hi"], "chrA", step, dict(CPM, low_memory=True)) for step in (50, 70, 30, 90, 110)],
    ("flag_include", ["mixed", "blocks"], "chrA", 50, dict(CPM, flag_include=16)),
    ("min_mapping_score", ["mixed", "longread"], "chrA", 50, dict(CPM, min_mapping_score=0)),
    ("extend_reads", ["mixed", "third_lo", "longread"], "chrA", 100, dict(CPM, extend_reads=150)),
    ("all_chrB", ["mixed", "blocks", "longread"], "chrB", 50, ONE_SET),
    ("all_chrA", ["mixed", "blocks", "longread"], "chrA", 50, ONE_SET),
    ("all_chrC", ["mixed", "blocks", "longread"], "chrC", 50, ONE_SET),
]
for name, files, contig, step, kwargs in SCENARIOS:
    if name.startswith("low_memory_odd_"):
        if "low_memory_odd_matrix" in arrays:
            continue
        _, matrix = rt.generate_chrom_matrix(contig, [BAMS[k] for k in files], SIZES, step, **kwargs)
        if matrix.shape[1] % 2 == 0:
            continue
        name = "low_memory_odd"
    entry = {"name": name, "files": files, "contig": contig, "step": step, "kwargs": dict(kwargs), "error": None, "none": False}
    try:
        (intervals, matrix), entry["log"] = logged(lambda: rt.generate_chrom_matrix(contig, [BAMS[k] for k in files], SIZES, step, **kwargs))
        entry["none"] = intervals is None
        if intervals is not None:
            arrays[f"{name}_intervals"], arrays[f"{name}_matrix"] = np.asarray(intervals), np.asarray(matrix)
    except (RuntimeError, ValueError) as exc:
        entry["error"], entry["error_type"], entry["log"] = str(exc).replace(SIZES, "{sizes}"), type(exc).__name__, logged.last
    meta["scenarios"].append(entry)
    print(name, "error: " + entry["error"] if entry["error"] else ("none" if entry["none"] else arrays[f"{name}_matrix"].shape), len(entry["log"]))

gap = arrays["gap_intervals"]
assert np.unique(np.diff(gap)).size > 1, "the union of third_lo and third_hi must have a gap"
step = 50
touch_rows = arrays["touch_matrix"]
touch = arrays["touch_intervals"]
last_a = touch[np.flatnonzero(touch_rows[0] > 0)[-1]]
first_b = touch[np.flatnonzero(touch_rows[1] > 0)[0]]
assert last_a + step == first_b and np.unique(np.diff(touch)).size == 1, (last_a, first_b)
assert any(e["none"] for e in meta["scenarios"]) and arrays["single_file_matrix"].shape[0] == 1
assert arrays["low_memory_matrix"].dtype == np.float32 and arrays["low_memory_odd_matrix"].dtype == np.float32
assert arrays["low_memory_odd_matrix"].shape[0] == 3 and arrays["low_memory_odd_matrix"].shape[1] % 2 == 1

np.savez_compressed(os.path.join(HERE, "bam_matrix.npz"), **arrays)
with open(os.path.join(HERE, "bam_matrix.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(meta['scenarios'])} scenarios, {len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'bam_matrix.npz'))} bytes")
