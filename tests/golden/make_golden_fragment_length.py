#!/usr/bin/env python3
"""What the REFERENCE's whole-file probes make of decoded alignment records.

    python tests/golden/make_golden_fragment_length.py        (by hand, where the reference is mounted; about 40 s)

Every stored value was written by the reference's compiled C or by its own Python function:

1. The reference's vendored htslib is built in a temporary directory exactly as make_golden_alignment_counts.py builds it
   (settings from the reference's own setup.py); the reference's ``native/ccounts_backend.c`` is compiled against it
   twice: with this project's tests/golden/fragment_length_driver.c (the four probes, the seven-field dump) and with
   tests/golden/alignment_counts_driver.c (``range`` / ``count``, for the end-to-end scenario).  Nothing built or copied
   there is kept.
2. SAM texts made from seeded random arrays become indexed BAM files; the driver dumps the seven fields of every record
   (the six of `AlignmentRecords` plus the query length) and calls ``ccounts_isPairedEnd``, ``ccounts_getReadLength``,
   ``ccounts_getMappedReadCount`` and ``ccounts_getFragmentLength`` with every parameter on its command line.
3. The reference's own ``_get_bam_count_metadata`` and ``get_bam_chrom_reads`` (rocco/readtracks.py:242-353, 389-518) run
   with ``_require_native_counter`` replaced IN THE MODULE by a stand-in whose methods call the drivers.

Writes tests/golden/fragment_length_vectors.npz + .json (data only)."""
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
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="fragment_length_")

# ---- 1. the reference's counter -------------------------------------------------------------------------------------
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
for binary, source in (("probe", "fragment_length_driver.c"), ("count", "alignment_counts_driver.c")):
    BINARIES[binary] = os.path.join(WORK, binary)
    subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS, "-I", os.path.join(REFERENCE, "rocco", "native"),
                    os.path.join(HERE, source), os.path.join(REFERENCE, "rocco", "native", "ccounts_backend.c"),
                    os.path.join(HTS, "libhts.a"), "-lz", "-lm", "-lpthread", "-o", BINARIES[binary]], check=True)


def driver(*args, binary="probe"):
    return subprocess.run([BINARIES[binary], *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout


# ---- 2. SAM texts from seeded random arrays ----------------------------------------------------------------------------
rng = np.random.default_rng(20257)
FIELDS = [("pos", np.int32), ("end", np.int32), ("isize", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("mate_same", np.uint8),
          ("qlen", np.int32)]
CIGARS = [("50M", 50, 50), ("50M", 50, 50), ("50M", 50, 50), ("36M", 36, 36), ("10S40M", 50, 40), ("20M5D30M", 50, 55), ("20M3I27M", 50, 47)]
arrays, meta = {}, {"files": {}, "paired": [], "readlen": [], "mapped": [], "fraglen": [], "metadata": [], "chrom_reads": []}
BAMS = {}


def sam_line(name, flag, contig, pos0, cigar, qlen, rnext="*", pnext=0, tlen=0, with_seq=True, mapq=30):
    seq = "A" * qlen if (with_seq and qlen > 0) else "*"
    return (int(pos0), f"{name}\t{flag}\t{contig}\t{int(pos0) + 1}\t{mapq}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t{seq}\t*")


def stranded(contig, length, centres, per_peak, cigars=CIGARS, fragment=(180.0, 20.0), spread=60.0, seq_rate=0.5, reverse_cigars=None):
    """Single-end reads with strand structure: fragments of length ~ N(fragment) clustered around `centres`; a fragment
    gives its forward read at its start or its reverse read ending at its end."""
    lines = []
    for centre in centres:
        starts = np.rint(centre + rng.normal(0.0, spread, size=per_peak)).astype(int)
        lengths = np.maximum(np.rint(rng.normal(fragment[0], fragment[1], size=per_peak)).astype(int), 2)
        for s, n in zip(starts, lengths):
            reverse = rng.random() < 0.5
            table = reverse_cigars if (reverse and reverse_cigars) else cigars
            cigar, qlen, reflen = table[int(rng.integers(0, len(table)))]
            pos0 = s + n - reflen if reverse else s
            if pos0 < 0 or pos0 + reflen > length:
                continue
            flag = (16 if reverse else 0) | (1024 if rng.random() < 0.05 else 0)
            lines.append(sam_line("s", flag, contig, pos0, cigar, qlen, with_seq=rng.random() < seq_rate))
    return lines


def uniform(contig, length, count, cigars=CIGARS, seq_rate=0.5):
    lines = []
    for pos0 in rng.integers(0, length - 60, size=count):
        cigar, qlen, _ = cigars[int(rng.integers(0, len(cigars)))]
        lines.append(sam_line("u", 16 if rng.random() < 0.5 else 0, contig, pos0, cigar, qlen, with_seq=rng.random() < seq_rate))
    return lines


def unmapped_placed(contig, length, count, qlen=50, seq_rate=0.5):
    """Unmapped records placed on a contig (at a mate's position): no CIGAR; SEQ present or `*` (query length 0)."""
    return [sam_line("x", 4 | (16 if rng.random() < 0.5 else 0), contig, pos0, "*", qlen, with_seq=rng.random() < seq_rate, mapq=0)
            for pos0 in rng.integers(0, length - 60, size=count)]


def pairs(contig, length, count, insert=(220.0, 40.0), read=50, improper=0.1, elsewhere=0.05, seq_rate=0.5):
    """Both mates of `count` templates; some improper, some with the mate on another contig or unmapped, TLEN of either
    sign (read 1 on either strand), a few outside any insert window."""
    lines = []
    for start in rng.integers(0, length - 1500, size=count):
        tlen = int(max(read, np.rint(rng.normal(*insert))))
        if rng.random() < 0.05:
            tlen = int(rng.integers(1001, 1400))
        left, right = int(start), int(start) + tlen - read
        proper = 0 if rng.random() < improper else 2
        first_left = rng.random() < 0.5
        rnext, mate_unmapped = "=", 0
        if rng.random() < elsewhere:
            rnext = "chrB" if contig != "chrB" else "chrA"
        elif rng.random() < 0.03:
            mate_unmapped = 8
        base = 1 | proper | mate_unmapped
        seq = rng.random() < seq_rate
        lines.append(sam_line("p", base | 32 | (64 if first_left else 128), contig, left, f"{read}M", read, rnext, right + 1, tlen, seq))
        if rnext == "=" and not mate_unmapped:
            lines.append(sam_line("p", base | 16 | (128 if first_left else 64), contig, right, f"{read}M", read, rnext, left + 1, -tlen, seq))
    return lines


def make_file(key, contigs, per_contig):
    """contigs: [(name, length)] in header order; per_contig: {name: [(pos0, line)]}.  Stores the decoded records."""
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in contigs:
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for name, _ in contigs:
            for _, line in sorted(per_contig.get(name, []), key=lambda item: item[0]):
                handle.write(line + "\n")
    driver("sam2bam", sam, bam)
    meta["files"][key] = {"contigs": [[name, int(length)] for name, length in contigs], "records": {}}
    for name, _ in contigs:
        out = os.path.join(WORK, f"{key}_{name}.txt")
        driver("dump", bam, name, out)
        with open(out) as handle:
            text = handle.read().split()
        table = np.asarray(text, dtype=np.int64).reshape(-1, 7)
        for column, (field, dtype) in enumerate(FIELDS):
            arrays[f"f_{key}_{name}_{field}"] = table[:, column].astype(dtype)
        meta["files"][key]["records"][name] = int(table.shape[0])
    BAMS[key] = bam
    return bam


def centres_on(length, count, margin=1500):
    return np.sort(rng.integers(margin, length - margin, size=count))


# header order differs from length order; chrB and chrC are equal in length (the first of equals stays ahead); chrS is
# shorter than any block
PEAK_CONTIGS = [("chrD", 60000), ("chrB", 120000), ("chrA", 400000), ("chrC", 120000), ("chrS", 2000)]
make_file("se_peaks", PEAK_CONTIGS, {
    "chrA": stranded("chrA", 400000, centres_on(400000, 22), 60) + unmapped_placed("chrA", 400000, 30),
    "chrB": stranded("chrB", 120000, centres_on(120000, 7), 60),
    "chrC": stranded("chrC", 120000, centres_on(120000, 7), 60),
    # (the head of the file: 40 unmapped records with a 75-base SEQ lead it, so excluding flag 4 changes the read length)
    "chrD": unmapped_placed("chrD", 60000, 12) + unmapped_placed("chrD", 600, 40, qlen=75, seq_rate=1.0) + stranded("chrD", 60000, centres_on(60000, 3), 50, cigars=[("36M", 36, 36)],
                                                                reverse_cigars=[("50M", 50, 50)]),  # (the head of the file)
    "chrS": uniform("chrS", 2000, 10)})
# reads without SEQ anywhere: every query length comes from the CIGAR
make_file("se_noseq", PEAK_CONTIGS, {
    "chrA": stranded("chrA", 400000, centres_on(400000, 12), 50, seq_rate=0.0),
    "chrB": stranded("chrB", 120000, centres_on(120000, 4), 50, seq_rate=0.0)})
# short reads in dense clusters: blocks of 64 and 257 bp hold ten reads per strand
DENSE_CONTIGS = [("chrA", 20000), ("chrB", 8000), ("chrC", 8000), ("chrD", 2000)]
SHORT = [("20M", 20, 20), ("20M", 20, 20), ("5S15M", 20, 15), ("18M", 18, 18)]
make_file("se_dense", DENSE_CONTIGS, {
    "chrA": stranded("chrA", 20000, centres_on(20000, 7, 400), 380, cigars=SHORT, fragment=(42.0, 4.0), spread=12.0),
    "chrB": stranded("chrB", 8000, centres_on(8000, 3, 400), 300, cigars=SHORT, fragment=(42.0, 4.0), spread=12.0),
    "chrC": stranded("chrC", 8000, centres_on(8000, 3, 400), 300, cigars=SHORT, fragment=(42.0, 4.0), spread=12.0),
    "chrD": uniform("chrD", 2000, 40, cigars=SHORT)})
make_file("se_uniform", PEAK_CONTIGS, {"chrA": uniform("chrA", 200000, 1800), "chrB": uniform("chrB", 60000, 500),
                                       "chrC": uniform("chrC", 60000, 500)})
# every block has fewer than ten reads on a strand
make_file("se_sparse", PEAK_CONTIGS, {"chrA": uniform("chrA", 400000, 150), "chrB": uniform("chrB", 120000, 40),
                                      "chrD": uniform("chrD", 60000, 40)})
# the second and third longest contigs are shorter than the default block
make_file("se_short", [("chrA", 30000), ("chrS", 3000), ("chrT", 2000)], {
    "chrA": stranded("chrA", 30000, centres_on(30000, 3), 60), "chrS": uniform("chrS", 3000, 200), "chrT": uniform("chrT", 2000, 100)})
PAIR_CONTIGS = [("chrB", 120000), ("chrA", 400000), ("chrC", 90000)]
PE = {"chrA": pairs("chrA", 400000, 450), "chrB": pairs("chrB", 120000, 200), "chrC": pairs("chrC", 90000, 100)}
make_file("pe_a", PAIR_CONTIGS, PE)
# one qualifying template more (its read 1; read 2 never counts): the other parity of the median
ONE_MORE = [sam_line("q", 1 | 2 | 32 | 64, "chrA", 1000, "50M", 50, "=", 1151, 200), sam_line("q", 1 | 2 | 16 | 128, "chrA", 1150, "50M", 50, "=", 1001, -200)]
make_file("pe_b", PAIR_CONTIGS, dict(PE, chrA=PE["chrA"] + ONE_MORE))
make_file("pe_many", PAIR_CONTIGS, {"chrA": pairs("chrA", 400000, 2100), "chrB": pairs("chrB", 120000, 700)})
# unpaired records lead the file (chrB is first in the header), pairs follow
make_file("mixed", PAIR_CONTIGS, {"chrB": uniform("chrB", 120000, 1200), "chrA": uniform("chrA", 400000, 600) + pairs("chrA", 400000, 300)})
make_file("empty", PAIR_CONTIGS, {})

# ---- the probes ----------------------------------------------------------------------------------------------------------
for key in BAMS:
    for max_reads in (1, 10, 1000, 1024, 0):
        meta["paired"].append({"file": key, "max_reads": max_reads, "paired": int(driver("paired", BAMS[key], max_reads))})
    for min_reads, max_iterations, flag_exclude in [(32, 4096, 0), (32, 4096, 16), (32, 4096, 4), (1, 1, 0), (0, 0, 0), (5, 3, 0), (33, 40, 1024),
                                                   (4096, 4096, 0), (32, 4096, 3844), (32, 4096, 65535), (7, 10, 20)]:
        text = driver("readlen", BAMS[key], min_reads, max_iterations, flag_exclude).strip()
        meta["readlen"].append({"file": key, "min_reads": min_reads, "max_iterations": max_iterations, "flag_exclude": flag_exclude,
                                "error": text[6:] if text.startswith("ERROR ") else None,
                                "read_length": None if text.startswith("ERROR ") else int(text)})
    for exclude in ([], ["chrA"], ["chrB", "chrS", "chrQ"], ["chrA", "chrB", "chrC", "chrD", "chrS", "chrT"]):
        mapped, unmapped = driver("mapped", BAMS[key], *exclude).split()
        meta["mapped"].append({"file": key, "exclude": exclude, "mapped": int(mapped), "unmapped": int(unmapped)})

DEFAULT = dict(flag_exclude=0, max_iterations=1000, max_insert_size=1000, block_size=5000, rolling_chunk_size=250, lag_step=5,
               early_exit=250, fallback=0)


def fraglen(key, **params):
    p = dict(DEFAULT, **params)
    value = int(driver("fraglen", BAMS[key], p["flag_exclude"], p["max_iterations"], p["max_insert_size"], p["block_size"],
                       p["rolling_chunk_size"], p["lag_step"], p["early_exit"], p["fallback"]))
    meta["fraglen"].append({"file": key, "params": params, "fragment_length": value})
    return value


for key in BAMS:
    fraglen(key)
    fraglen(key, max_iterations=4096)  # (what _estimate_fragment_length asks for)
    fraglen(key, fallback=147)
    fraglen(key, flag_exclude=65535, fallback=147)
    fraglen(key, flag_exclude=65535)
    fraglen(key, flag_exclude=16)
    fraglen(key, flag_exclude=1024, lag_step=1, max_iterations=8)
for key in ("se_noseq", "se_short"):
    fraglen(key, lag_step=7, block_size=1000)
    fraglen(key, rolling_chunk_size=100, max_iterations=3, early_exit=4)
    fraglen(key, max_insert_size=30)
    fraglen(key, max_insert_size=6000, lag_step=7, max_iterations=12)
for key in ("se_peaks", "se_uniform"):
    for lag_step in (1, 5, 7):
        for block_size in (1000, 5000):
            fraglen(key, lag_step=lag_step, block_size=block_size, max_iterations=12)
    for chunk in (1, 100, 250, 7000):
        fraglen(key, rolling_chunk_size=chunk)
        fraglen(key, rolling_chunk_size=chunk, max_iterations=3, lag_step=7)
    for max_iterations in (1, 3, 1000):
        for early_exit in (0, 1, 3, 4, 5, 250):
            fraglen(key, max_iterations=max_iterations, early_exit=early_exit, lag_step=1 if max_iterations == 3 else 5)
    fraglen(key, max_insert_size=30)
    fraglen(key, max_insert_size=30, fallback=147)
    fraglen(key, max_insert_size=6000, lag_step=7, max_iterations=12)
    fraglen(key, max_insert_size=100, lag_step=1)
    fraglen(key, max_insert_size=0, block_size=0, rolling_chunk_size=0, lag_step=0, max_iterations=0, early_exit=-3)
for block_size in (10, 64, 257, 1000, 5000):
    for lag_step in (1, 5, 7):
        fraglen("se_dense", block_size=block_size, lag_step=lag_step)
        fraglen("se_dense", block_size=block_size, lag_step=lag_step, rolling_chunk_size=100, max_iterations=3, early_exit=4)
    fraglen("se_dense", block_size=block_size, rolling_chunk_size=1, lag_step=1, max_iterations=3)
    fraglen("se_dense", block_size=block_size, max_insert_size=1000, lag_step=1, early_exit=1)
    fraglen("se_dense", block_size=block_size, rolling_chunk_size=block_size + 36, lag_step=1)
    fraglen("se_dense", block_size=block_size, max_insert_size=12)
for key in ("pe_a", "pe_b", "pe_many", "mixed"):
    for max_iterations in (1, 3, 1000, 2500):
        fraglen(key, max_iterations=max_iterations)
    fraglen(key, max_insert_size=200)
    fraglen(key, max_insert_size=20)
    fraglen(key, flag_exclude=64)
    fraglen(key, flag_exclude=1)

# ---- 3. the reference's own _get_bam_count_metadata / get_bam_chrom_reads over a stand-in native module --------------
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco")]
sys.modules["rocco"] = pkg
rt = importlib.import_module("rocco.readtracks")


class Native:
    """The compiled counter's methods (rocco/_hts_counts.c: names, keywords and defaults), answered by the drivers."""

    def is_alignment_paired_end(self, bam, max_reads=1000, thread_count=0):
        return bool(int(driver("paired", bam, max_reads)))

    def get_alignment_read_length(self, bam, min_reads=32, thread_count=0, max_iterations=4096, flag_exclude=0):
        text = driver("readlen", bam, min_reads, max_iterations, flag_exclude).strip()
        if text.startswith("ERROR "):
            raise RuntimeError(text[6:])
        return int(text)

    def get_alignment_mapped_read_count(self, bam, exclude_chromosomes=(), thread_count=0, count_mode="coverage", one_read_per_bin=0):
        mapped, unmapped = driver("mapped", bam, *exclude_chromosomes).split()
        return int(mapped), int(unmapped)

    def get_alignment_fragment_length(self, bam, thread_count=0, flag_exclude=0, max_iterations=1000, max_insert_size=1000,
                                      block_size=5000, rolling_chunk_size=250, lag_step=5, early_exit=250, fallback=0):
        return int(driver("fraglen", bam, flag_exclude, max_iterations, max_insert_size, block_size, rolling_chunk_size, lag_step,
                          early_exit, fallback))

    def get_alignment_chrom_range(self, bam, chromosome, chrom_size, thread_count=1, flag_exclude=0):
        a, b = driver("range", bam, chromosome, chrom_size, flag_exclude, binary="count").split()
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


def logged(call, bam):
    keep = Keep()
    rt.logger.addHandler(keep)
    rt._BAM_COUNT_METADATA_CACHE.clear()
    try:
        result = call()
    finally:
        rt.logger.removeHandler(keep)
    return result, [[level, message.replace(bam, "{file}")] for level, message in keep.records]


def metadata_scenario(key, step=50, norm_method="RPGC", effective_genome_size=2.7e9, ignore_for_norm=None, flag_exclude=0,
                      extend_reads=-1, scale_factor=1.0):
    call = dict(step=step, norm_method=norm_method, effective_genome_size=effective_genome_size, ignore_for_norm=ignore_for_norm,
                flag_exclude=flag_exclude, extend_reads=extend_reads, scale_factor=scale_factor)
    try:
        metadata, log = logged(lambda: rt._get_bam_count_metadata(BAMS[key], num_processors=1, **call), BAMS[key])
        metadata = {k: v for k, v in metadata.items() if k != "threads"}
        error = None
    except RuntimeError as exc:
        metadata, log, error = None, [], str(exc)
    meta["metadata"].append({"file": key, "call": call, "metadata": metadata, "log": log, "error": error})


for key in BAMS:
    for extend_reads in (-1, 0, 150):
        metadata_scenario(key, extend_reads=extend_reads)
    metadata_scenario(key, extend_reads=0, flag_exclude=3844, norm_method="CPM", ignore_for_norm=["chrB", "chrM"], scale_factor=2.5)
    metadata_scenario(key, extend_reads=0, flag_exclude=16, norm_method="RPKM", step=200)
    if key.startswith("pe_"):
        metadata_scenario(key, extend_reads=0, flag_exclude=64)  # paired, and no template qualifies

SIZES = os.path.join(WORK, "t.sizes")
for key, contig, extend_reads in [("se_peaks", "chrA", 0), ("se_peaks", "chrB", -1), ("pe_a", "chrA", 0), ("se_uniform", "chrC", 0)]:
    with open(SIZES, "w") as handle:
        for name, length in meta["files"][key]["contigs"]:
            handle.write(f"{name}\t{length}\n")
    kwargs = dict(effective_genome_size=2.7e9, norm_method="RPGC", min_mapping_score=10, flag_include=None, flag_exclude=3844,
                  extend_reads=extend_reads, center_reads=False, ignore_for_norm=["chrS"], scale_factor=1.0, num_processors=1,
                  const_scale=1.0, round_digits=5, scale_by_step=False)
    (intervals, vals), log = logged(lambda: rt.get_bam_chrom_reads(BAMS[key], contig, SIZES, 50, **kwargs), BAMS[key])
    name = f"{key}_{contig}"
    arrays[f"r_{name}_intervals"], arrays[f"r_{name}_values"] = np.asarray(intervals), np.asarray(vals)
    meta["chrom_reads"].append({"name": name, "file": key, "contig": contig, "step": 50, "kwargs": kwargs, "log": log})

np.savez_compressed(os.path.join(HERE, "fragment_length_vectors.npz"), **arrays)
with open(os.path.join(HERE, "fragment_length_vectors.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(meta['paired'])} paired, {len(meta['readlen'])} readlen, {len(meta['mapped'])} mapped, {len(meta['fraglen'])} fraglen, "
      f"{len(meta['metadata'])} metadata and {len(meta['chrom_reads'])} chrom_reads scenarios, {len(arrays)} arrays, "
      f"{os.path.getsize(os.path.join(HERE, 'fragment_length_vectors.npz'))} bytes")
for r in meta["fraglen"]:
    print("  fraglen", r["file"], r["params"], "->", r["fragment_length"])
for r in meta["metadata"]:
    print("  metadata", r["file"], r["call"]["extend_reads"], r["metadata"], r["log"], r["error"])
