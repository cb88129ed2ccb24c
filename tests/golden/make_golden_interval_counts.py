#!/usr/bin/env python3
"""What the REFERENCE makes of decoded alignment records over peaks and null regions.

    python tests/golden/make_golden_interval_counts.py        (by hand, where the reference is mounted; a few minutes)

Every stored value was written by the reference's compiled C or by its own Python functions:

1. The reference's counter is built over its vendored htslib exactly as make_golden_alignment_counts.py builds it, with
   this project's driver (tests/golden/alignment_counts_driver.c, unchanged).  The driver's ``count`` command with
   ``length = 1`` and ``intervalSizeBP = end - start`` is one interval of the reference's ``count_alignment_intervals``
   (rocco/_hts_counts.c:808-818).  Nothing built or copied there is kept.
2. Three small BAM files from seeded SAM text over three contigs (one without records); the decoded records are stored.
3. About 300 intervals per contig, counted per file under five option sets.
4. The reference's own ``raw_count_matrix``, ``_random_intervals``, ``_assign_length_bins``, ``_read_peak_intervals``,
   ``get_ecdf`` and ``score_peaks`` (rocco/scores.py) run as they are, with ``_hts_counts`` replaced IN THE MODULE by a
   stand-in that calls the driver, a stand-in ``pysam`` module whose ``AlignmentFile.count(chrom, start, end,
   read_callback)`` goes to the driver at the options that equal pysam's rule (flag_exclude=4, min_mapping_quality=10,
   one_read_per_bin=1; argued in DESIGN.md note (27), pysam itself is not installed) and whose ``.mapped`` /
   ``.count(chrom)`` return prepared numbers, and ``get_read_length`` replaced in the module.

Writes tests/golden/interval_count_vectors.npz + .json (data only)."""
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="interval_counts_")

# ---- 1. the reference's counter (as make_golden_alignment_counts.py) ---------------------------------------------------
HTS = os.path.join(WORK, "htslib")
shutil.copytree(os.path.join(REFERENCE, "vendor", "htslib"), HTS)


def reference_build_settings():
    """The reference's own setup.py says how its vendored htslib is configured without ``configure`` and with which flags
    its extensions are compiled: only its imports, module-level assignments and functions are executed."""
    import ast

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
DRIVER = os.path.join(WORK, "driver")
subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS,
                "-I", os.path.join(REFERENCE, "rocco", "native"), os.path.join(HERE, "alignment_counts_driver.c"),
                os.path.join(REFERENCE, "rocco", "native", "ccounts_backend.c"), os.path.join(HTS, "libhts.a"),
                "-lz", "-lm", "-lpthread", "-o", DRIVER], check=True)


def driver(*args):
    return subprocess.run([DRIVER, *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout


# ---- 2. SAM texts from seeded random arrays ----------------------------------------------------------------------------
rng = np.random.default_rng(20261)
CIGARS = [("50M", 50), ("50M", 50), ("50M", 50), ("20M5D30M", 55), ("10S40M", 40), ("25M100N25M", 150), ("20M3I27M", 47),
          ("36M", 36), ("5S30M400N30M5S", 460), ("*", 1)]
CONTIGS = {"chrA": 120000, "chrB": 50000, "chrE": 20000}
PILE = 61000
arrays, meta = {}, {"contigs": CONTIGS, "files": {}, "options": {}, "pile_position": PILE}


def sam_lines(contig, pos, plain=None):
    """One SAM line per position (the generator of make_golden_alignment_counts.py): both strands, proper / improper pairs
    of either TLEN sign, mates elsewhere, secondary, duplicate and unmapped-but-placed records, every mapping quality,
    zero-length and spliced CIGARs.  ``plain[i]``: a 50M read (the pile-up)."""
    lines = []
    for i, p in enumerate(pos):
        cigar, _ = CIGARS[int(rng.integers(0, len(CIGARS)))]
        flag = 16 if rng.random() < 0.5 else 0
        rnext, pnext, tlen = "*", 0, 0
        if rng.random() < 0.55:
            flag |= 1 | (2 if rng.random() < 0.85 else 0) | (64 if rng.random() < 0.5 else 128) | (32 if not flag & 16 else 0)
            tlen = int(rng.integers(20, 900)) * (1 if rng.random() < 0.5 else -1)
            if rng.random() < 0.04:
                tlen = 0
            rnext, pnext = ("=" if rng.random() < 0.93 else "chrB" if contig != "chrB" else "chrA"), int(max(1, p + tlen))
            if rng.random() < 0.04:
                flag |= 8
        if rng.random() < 0.04:
            flag |= 256
        if rng.random() < 0.04:
            flag |= 1024
        if rng.random() < 0.03:
            flag, cigar = flag | 4, "*"  # unmapped, placed at its mate's position
        mapq = int(rng.integers(0, 61)) if rng.random() < 0.8 else int(rng.choice([0, 9, 10, 11, 29, 30, 31, 255]))
        if plain is not None and plain[i]:
            cigar = "50M"
        lines.append(f"r{i}\t{flag}\t{contig}\t{int(p) + 1}\t{mapq}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t*\t*")
    return lines


def make_file(key, positions):
    """positions: {contig: (sorted positions, plain mask or None)}.  Stores the decoded records of every contig."""
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in CONTIGS.items():
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for name in CONTIGS:
            if name in positions:
                for line in sam_lines(name, *positions[name]):
                    handle.write(line + "\n")
    driver("sam2bam", sam, bam)
    meta["files"][key] = {}
    for name in CONTIGS:
        out = os.path.join(WORK, f"{key}_{name}.txt")
        driver("dump", bam, name, out)
        table = np.loadtxt(out, dtype=np.int64, ndmin=2).reshape(-1, 6)
        for column, (field, dtype) in enumerate([("pos", np.int32), ("end", np.int32), ("isize", np.int32), ("flag", np.uint16),
                                                  ("mapq", np.uint8), ("mate_same", np.uint8)]):
            arrays[f"f_{key}_{name}_{field}"] = table[:, column].astype(dtype)
        meta["files"][key][name] = int(table.shape[0])
    return bam


def with_pile(n, depth):
    """n ragged positions between 2 000 and 117 000 (nothing at either end of the contig) and `depth` reads on PILE."""
    pos = np.concatenate([rng.integers(2000, 117000, size=n), np.full(depth, PILE)])
    plain = np.concatenate([np.zeros(n, dtype=bool), np.ones(depth, dtype=bool)])
    order = np.argsort(pos, kind="stable")
    return pos[order], plain[order]


BAMS = {
    "s1": make_file("s1", {"chrA": with_pile(16500, 3500), "chrB": (np.sort(rng.integers(0, 49990, size=1500)), None)}),
    "s2": make_file("s2", {"chrA": with_pile(3200, 300), "chrB": (np.sort(rng.integers(500, 49000, size=900)), None)}),
    "s3": make_file("s3", {"chrA": (np.sort(rng.integers(0, 119990, size=2500)), None),
                           "chrB": (np.sort(rng.integers(0, 49990, size=700)), None)}),
}
FILES = list(BAMS)

DEFAULTS = dict(one_read_per_bin=0, flag_include=0, flag_exclude=0, shift_forward_strand53=0, shift_reverse_strand53=0,
                extend_bp=0, max_insert_size=1000, paired_end_mode=0, min_mapping_quality=0, min_template_length=-1, read_length=0)
_tls = threading.local()


def interval_count(bam, contig, start, end, **options):
    """One interval of count_alignment_intervals: region [start, end), intervalSizeBP = end - start, a buffer of one float."""
    o = dict(DEFAULTS, **options)
    if getattr(_tls, "pid", None) != os.getpid():  # (multi_ecdf forks: one output file per process and thread)
        _tls.pid, _tls.out = os.getpid(), os.path.join(WORK, f"count_{os.getpid()}_{threading.get_ident()}.f32")
    driver("count", bam, contig, start, end, end - start, 1, 0, _tls.out, o["one_read_per_bin"], o["flag_include"],
           o["flag_exclude"], o["shift_forward_strand53"], o["shift_reverse_strand53"], o["read_length"], o["extend_bp"],
           o["min_mapping_quality"], o["min_template_length"], o["max_insert_size"], o["paired_end_mode"])
    return float(np.fromfile(_tls.out, dtype=np.float32)[0])


POOL = ThreadPoolExecutor(16)


def interval_counts(bam, chroms, starts, ends, **options):
    return np.asarray(list(POOL.map(lambda a: interval_count(bam, a[0], int(a[1]), int(a[2]), **options), zip(chroms, starts, ends))),
                      dtype=np.float32)


# ---- 3. intervals ---------------------------------------------------------------------------------------------------------
OPTION_SETS = {
    "raw_count_matrix": dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10),
    "null": dict(one_read_per_bin=1, flag_exclude=4, min_mapping_quality=10),
    "paired": dict(one_read_per_bin=1, paired_end_mode=1, read_length=50, flag_exclude=3844, min_mapping_quality=10),
    "extend_shift": dict(one_read_per_bin=1, extend_bp=150, shift_forward_strand53=4, shift_reverse_strand53=5, flag_exclude=3844),
    "coverage_cells": dict(one_read_per_bin=0, flag_exclude=1796),
}
meta["options"] = OPTION_SETS


def make_intervals(contig, size, count):
    starts, ends = [], []
    widths = np.unique(np.round(np.exp(rng.uniform(0, np.log(size), size=count - 60))).astype(np.int64))
    for w in np.concatenate([[1, 1, 2, size, size], widths]):
        s = int(rng.integers(0, size - w + 1))
        starts.append(s)
        ends.append(s + int(w))
    for _ in range(12):  # nested in, and overlapping, the ones before
        k = int(rng.integers(0, len(starts)))
        s, e = starts[k], ends[k]
        if e - s >= 4:
            starts += [s + (e - s) // 4, s + (e - s) // 2]
            ends += [e - (e - s) // 4, e + (e - s) // 2]
    for _ in range(10):  # repeated
        k = int(rng.integers(0, len(starts)))
        starts.append(starts[k])
        ends.append(ends[k])
    # before the first record, behind the last one, ending past the contig
    starts += [0, 0, 10, size - 40, size - 1, size - 1000, size - 3000, 0]
    ends += [1, 1500, 1999, size, size, size + 500, size + 1, size + 100000]
    if contig == "chrA":  # cutting the pile-up
        for s, e in [(PILE, PILE + 1), (PILE - 1, PILE), (PILE + 1, PILE + 2), (PILE - 10, PILE), (PILE - 10, PILE + 1), (PILE, PILE + 50),
                     (PILE + 49, PILE + 50), (PILE + 50, PILE + 60), (PILE - 49, PILE + 1), (PILE - 200, PILE + 25), (PILE + 25, PILE + 400),
                     (PILE - 150, PILE - 100), (PILE + 100, PILE + 200), (PILE - 5000, PILE + 5000)]:
            starts.append(s)
            ends.append(e)
    order = rng.permutation(len(starts))
    return np.asarray(starts, dtype=np.int64)[order], np.asarray(ends, dtype=np.int64)[order]


for contig, size in CONTIGS.items():
    starts, ends = make_intervals(contig, size, 370)
    arrays[f"iv_{contig}_start"], arrays[f"iv_{contig}_end"] = starts, ends
    for option_name, options in OPTION_SETS.items():
        for key in FILES:
            arrays[f"c_{option_name}_{key}_{contig}"] = interval_counts(BAMS[key], [contig] * len(starts), starts, ends, **options)
    print("counted", contig, len(starts), "intervals", flush=True)

# ---- 4. the reference's own Python over stand-ins ----------------------------------------------------------------------------
MAPPED = {"s1": 21000, "s2": 4400, "s3": 3100}
SKIPPED = {"s1": {"chrE": 0}, "s2": {"chrE": 0}, "s3": {"chrE": 0}}
READ_LENGTHS = {"s1": 50, "s2": 47, "s3": 36}
KEY_OF = {path: key for key, path in BAMS.items()}


class AlignmentFile:
    """pysam.AlignmentFile as rocco/scores.py uses it."""

    def __init__(self, path, mode="rb", threads=1):
        self.key = KEY_OF[path]
        self.path = path
        self.mapped = MAPPED[self.key]

    def count(self, contig=None, start=None, stop=None, read_callback=None):
        if start is None:
            return SKIPPED[self.key].get(contig, 0)
        # _check_read: mapped and mapping_quality >= 10, over what the index iterator yields
        return int(interval_count(self.path, contig, int(start), int(stop), **OPTION_SETS["null"]))

    def close(self):
        pass


pysam = types.ModuleType("pysam")
pysam.AlignmentFile = AlignmentFile
pysam.AlignedSegment = object
sys.modules["pysam"] = pysam
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco")]
sys.modules["rocco"] = pkg
sc = importlib.import_module("rocco.scores")


class Native:
    def count_alignment_intervals(self, bam, chroms, starts, ends, thread_count=1, count_mode="coverage", **options):
        assert count_mode == "coverage"
        return interval_counts(bam, chroms, starts, ends, **options)


sc._hts_counts = Native()
sc.get_read_length = lambda bam, *a, **k: READ_LENGTHS[KEY_OF[bam]]

SIZES = os.path.join(WORK, "g.sizes")
with open(SIZES, "w") as handle:
    for name, length in CONTIGS.items():
        handle.write(f"{name}\t{length}\n")
meta["sizes_text"] = open(SIZES).read()

# peaks: lengths 150 .. 3 000 bp on chrA and chrB, some on the pile-up, one on the empty contig
peak_rows = []
for _ in range(150):
    contig = "chrA" if rng.random() < 0.75 else "chrB"
    length = int(rng.integers(150, 3000))
    start = int(rng.integers(0, CONTIGS[contig] - length))
    peak_rows.append((contig, start, start + length))
peak_rows += [("chrA", PILE - 300, PILE + 400), ("chrA", PILE, PILE + 180), ("chrE", 5000, 5600), ("chrA", 100, 700)]
peak_rows.sort(key=lambda r: (r[0], r[1]))
PEAKS = os.path.join(WORK, "peaks.bed")
with open(PEAKS, "w") as handle:
    for row in peak_rows:
        handle.write("\t".join(str(v) for v in row) + "\n")
    handle.write("\n")
meta["peaks_text"] = open(PEAKS).read()

chroms, starts, ends, bed_strings, names = sc._read_peak_intervals(PEAKS, min_columns=3)
meta["read_peak_intervals"] = {"chroms": chroms, "starts": starts, "ends": ends, "bed_strings": bed_strings, "names": names}
SHORT = os.path.join(WORK, "short.bed")
with open(SHORT, "w") as handle:
    handle.write("chrA\t5\t9\tname\nchrA\t7\n")
try:
    sc._read_peak_intervals(SHORT, min_columns=3)
except ValueError as error:
    meta["read_peak_intervals_error"] = {"text": "chrA\t5\t9\tname\nchrA\t7\n", "min_columns": 3, "message": str(error)}
try:
    sc._read_peak_intervals(PEAKS, min_columns=5)
except ValueError as error:
    meta["read_peak_intervals_error5"] = {"min_columns": 5, "message": str(error)}

BAM_LIST = [BAMS[k] for k in FILES]
TSV = os.path.join(WORK, "counts.tsv")
sc.raw_count_matrix(BAM_LIST, PEAKS, TSV, bed_columns=3)
arrays["raw_count_matrix_tsv"] = np.frombuffer(open(TSV, "rb").read(), dtype=np.uint8)
meta["sample_names"] = FILES

meta["random_intervals"] = []
for seed, length, nsamples in [(1, 200, 20), (7, 1, 15), (7, 19999, 25), (42, 20001, 30), (42, 50000, 10), (3, 119999, 5), (5, 0, 4),
                               (11, 731, 0)]:
    out = sc._random_intervals(SIZES, length=length, nsamples=nsamples, seed=seed)
    meta["random_intervals"].append({"seed": seed, "length": length, "nsamples": nsamples, "intervals": [list(t) for t in out]})
try:
    sc._random_intervals(SIZES, length=120001, nsamples=5, seed=1)
except ValueError as error:
    meta["random_intervals_error"] = {"length": 120001, "message": str(error).replace(SIZES, "{file}")}

meta["assign_length_bins"] = []
peak_lengths = np.asarray([e - s for s, e in zip(starts, ends)], dtype=np.float64)
for label, lengths, max_bins, width in [("peaks24", peak_lengths, 24, 100), ("peaks5", peak_lengths, 5, 100), ("peaks_wide", peak_lengths, 24, 1000),
                                        ("few", np.asarray([300.0, 300.0, 500.0]), 24, 100), ("one", np.asarray([250.0]), 24, 100),
                                        ("narrow", np.asarray([200.0, 210.0, 220.0, 260.0, 0.0]), 24, 100),
                                        ("dense", np.arange(100, 1200, 7, dtype=np.float64), 6, 100)]:
    binned, reps = sc._assign_length_bins(lengths, max_bins=max_bins, min_bin_width_bp=width)
    arrays[f"alb_{label}_lengths"], arrays[f"alb_{label}_binned"], arrays[f"alb_{label}_reps"] = lengths, binned, reps
    meta["assign_length_bins"].append({"name": label, "max_bins": max_bins, "min_bin_width_bp": width})
try:
    sc._assign_length_bins(np.zeros(0))
except ValueError as error:
    meta["assign_length_bins_error"] = str(error)

# get_ecdf on its own: with scaling constants, and with a trimmed right tail
meta["get_ecdf"] = []
for label, kwargs in [("plain", dict(length=400, nsamples=60, sample_scaling_constants=None, seed=5)),
                      ("scaled_trimmed", dict(length=1500, nsamples=80, sample_scaling_constants=[2.5, 11.25, 30.5], seed=9,
                                              trim_proportion=0.1, row_scale=500.0, pc=0.5))]:
    null = sc.get_ecdf(BAM_LIST, chrom_sizes_file=SIZES, **kwargs)
    arrays[f"ecdf_{label}_values"] = null.values
    meta["get_ecdf"].append({"name": label, "kwargs": kwargs})

# the whole score_peaks
SUMMITS = os.path.join(WORK, "summits.tsv")
with open(SUMMITS, "w") as handle:
    handle.write(f"{names[0]}\t17\n{names[5]}\t999999\n\n{names[9]}\t0\n")
meta["summit_offsets_text"] = open(SUMMITS).read()
SCORED = os.path.join(WORK, "scored.bed")
TSV2 = os.path.join(WORK, "counts_for_scores.tsv")
score_kwargs = dict(effective_genome_size=2.7e6, skip_for_norm=["chrE"], row_scale=1000, ucsc_base=250, pc=1, ecdf_nsamples=50,
                    ecdf_max_length_bins=6, seed=77)
scores, bed6, pvals = sc.score_peaks(BAM_LIST, chrom_sizes_file=SIZES, peak_file=PEAKS, count_matrix_file=TSV2, output_file=SCORED,
                                     threads=1, proc=2, summit_offsets_file=SUMMITS, **score_kwargs)
assert open(TSV2, "rb").read() == open(TSV, "rb").read()
arrays["score_peaks_narrowpeak"] = np.frombuffer(open(SCORED, "rb").read(), dtype=np.uint8)
arrays["score_peaks_scores"], arrays["score_peaks_bed6"], arrays["score_peaks_pvals"] = scores, np.asarray(bed6), pvals
meta["score_peaks"] = {"kwargs": score_kwargs, "mapped_counts": [MAPPED[k] - sum(SKIPPED[k].values()) for k in FILES],
                       "read_lengths": [READ_LENGTHS[k] for k in FILES]}
# the nulls score_peaks used: multi_ecdf as it was called there
mapped_sizes = np.asarray(meta["score_peaks"]["mapped_counts"]) * np.asarray(meta["score_peaks"]["read_lengths"])
constants = score_kwargs["effective_genome_size"] / mapped_sizes
binned, reps = sc._assign_length_bins(peak_lengths, max_bins=score_kwargs["ecdf_max_length_bins"])
nulls = sc.multi_ecdf(BAM_LIST, reps, SIZES, nsamples_per_length=score_kwargs["ecdf_nsamples"], sample_scaling_constants=constants,
                      seed=score_kwargs["seed"], proc=2, row_scale=score_kwargs["row_scale"], pc=score_kwargs["pc"])
arrays["score_peaks_null_lengths"] = np.asarray(list(nulls), dtype=np.int64)
for length, null in nulls.items():
    arrays[f"score_peaks_null_{int(length)}"] = null.values
arrays["score_peaks_constants"] = constants

np.savez_compressed(os.path.join(HERE, "interval_count_vectors.npz"), **arrays)
with open(os.path.join(HERE, "interval_count_vectors.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'interval_count_vectors.npz'))} bytes; "
      f"{len(reps)} length bins; files {meta['files']}")
