#!/usr/bin/env python3
"""What the REFERENCE makes of decoded alignment records.

    python tests/golden/make_golden_alignment_counts.py        (by hand, where the reference is mounted; about 30 s)

Every stored value was written by the reference's compiled C or by its own Python function:

1. The reference's vendored htslib is copied into a temporary directory, given the three small settings files a build
   without ``configure`` needs (config.mk, config.h, htscodecs' version.h: the reference's setup.py returns their text
   and its compile flags, which are taken from it when this runs), built with
   ``make -j16 lib-static``; the reference's ``native/ccounts_backend.c`` is compiled against it together with this
   project's driver (tests/golden/alignment_counts_driver.c).  Nothing built or copied there is kept.
2. SAM texts made from seeded random arrays become BAM files with an index (the driver's ``sam2bam``); the driver dumps
   the six fields of every record of a contig in file order (``dump``), calls ``ccounts_getChromRange`` (``range``) and
   ``ccounts_openSource`` / ``ccounts_countRegion`` (``count``).
3. The reference's own ``get_bam_chrom_reads`` (rocco/readtracks.py:389-518) runs with ``_require_native_counter``
   replaced IN THE MODULE by a stand-in whose methods return prepared whole-file values and, for
   ``get_alignment_chrom_range`` / ``count_alignment_region``, the driver's results.  ``_compute_native_scale_factor``
   is called as it is.

Writes tests/golden/alignment_count_vectors.npz + .json (data only)."""
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
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="alignment_counts_")

# ---- 1. the reference's counter -------------------------------------------------------------------------------------
HTS = os.path.join(WORK, "htslib")
shutil.copytree(os.path.join(REFERENCE, "vendor", "htslib"), HTS)


def reference_build_settings():
    """The reference's own setup.py says how its vendored htslib is configured without ``configure`` and with which flags
    its extensions are compiled.  Importing it would run ``setup()``, so only its imports, module-level assignments and
    functions are executed; what they return is written and used as it is, and nothing of it is kept here."""
    import ast

    path = os.path.join(REFERENCE, "setup.py")
    with open(path, encoding="utf-8") as handle:
        tree = ast.parse(handle.read(), path)
    scope = {"__file__": path, "__name__": "reference_setup"}
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom, ast.Assign, ast.AnnAssign, ast.FunctionDef)):
            try:
                exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
            except NameError:  # (an assignment that needs one of the classes left out: the extension list)
                pass
    return scope


SETTINGS = reference_build_settings()
for written, text in (("config.mk", SETTINGS["get_vendored_htslib_config_mk"]()), ("config.h", SETTINGS["get_vendored_htslib_config_h"]())):
    with open(os.path.join(HTS, written), "w", encoding="utf-8") as handle:
        handle.write(text)
SETTINGS["HTSCODECS_CONFIGURE_AC_PATH"] = os.path.join(HTS, "htscodecs", "configure.ac")  # (the copy; the same text)
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
rng = np.random.default_rng(20251)
CIGARS = [("50M", 50), ("50M", 50), ("50M", 50), ("20M5D30M", 55), ("10S40M", 40), ("25M100N25M", 150), ("20M3I27M", 47),
          ("36M", 36), ("5S30M400N30M5S", 460), ("*", 1)]
CONTIGS = {"chrT": 100000, "chrU": 40000, "chrE": 30000, "chrL": 3000000, "chrN": 2500000}
arrays, meta = {}, {"files": {}, "count": [], "range": [], "tail": [], "scale": []}


def sam_lines(contig, pos, pile=None):
    """One SAM line per position: both strands, proper / improper pairs of either TLEN sign, mates elsewhere, secondary,
    duplicate and unmapped-but-placed records, every mapping quality, CIGARs whose reference span is not the read length."""
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
            rnext, pnext = ("=" if rng.random() < 0.93 else "chrU"), int(max(1, p + tlen))
            if rng.random() < 0.04:
                flag |= 8
        if rng.random() < 0.04:
            flag |= 256
        if rng.random() < 0.04:
            flag |= 1024
        if rng.random() < 0.03:
            flag, cigar = flag | 4, "*"  # unmapped, placed at its mate's position
        mapq = int(rng.integers(0, 61)) if rng.random() < 0.8 else int(rng.choice([0, 9, 10, 11, 29, 30, 31, 255]))
        if pile is not None and i >= pile:
            cigar = "50M"
        lines.append(f"r{i}\t{flag}\t{contig}\t{int(p) + 1}\t{mapq}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t*\t*")
    return lines


def make_file(key, per_contig):
    """per_contig: {contig: lines}.  Returns the BAM path; stores the decoded records of every contig."""
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in CONTIGS.items():
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for name in CONTIGS:
            for line in per_contig.get(name, []):
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


# "main": 3 000 ragged records over chrT, reads hanging over both ends of the contig, a 3 000-deep pile-up in one bin
main_pos = np.sort(np.concatenate([rng.integers(0, 99990, size=2900), rng.integers(0, 40, size=50), rng.integers(99940, 99999, size=50),
                                   ]))
pile_pos = np.sort(rng.integers(61000, 61050, size=3000))
order = np.argsort(np.concatenate([main_pos, pile_pos]), kind="stable")
all_lines = np.array(sam_lines("chrT", main_pos) + sam_lines("chrT", pile_pos, pile=0), dtype=object)[order]
MAIN = make_file("main", {"chrT": list(all_lines), "chrU": sam_lines("chrU", np.sort(rng.integers(0, 39000, size=400)))})
# "big": about 20 000 records
BIG = make_file("big", {"chrT": sam_lines("chrT", np.sort(rng.integers(0, 99950, size=20000)))})
# "long": a contig longer than the 2 Mb tail cushion, reads at its head, a few in its last 2 Mb
LONG = make_file("long", {"chrL": sam_lines("chrL", np.sort(np.concatenate([rng.integers(5000, 400000, size=300),
                                                                             rng.integers(1200000, 1300000, size=40)])))})
# "noend": reads at the head of a contig only, none reaching into its last 2 Mb: a start without an end
NOEND = make_file("noend", {"chrN": sam_lines("chrN", np.sort(rng.integers(1000, 400000, size=200)))})
BAMS = {"main": MAIN, "big": BIG, "long": LONG, "noend": NOEND}

DEFAULTS = dict(one_read_per_bin=0, flag_include=0, flag_exclude=0, shift_forward_strand53=0, shift_reverse_strand53=0,
                extend_bp=0, max_insert_size=1000, paired_end_mode=0, min_mapping_quality=0, min_template_length=-1)


def reference_count(bam, contig, start, end, step, read_length, length=None, prefill=0, **options):
    o = dict(DEFAULTS, **options)
    length = ((end - start - 1) // step) + 1 if length is None else length
    out = os.path.join(WORK, "counts.f32")
    driver("count", bam, contig, start, end, step, length, prefill, out, o["one_read_per_bin"], o["flag_include"],
           o["flag_exclude"], o["shift_forward_strand53"], o["shift_reverse_strand53"], read_length, o["extend_bp"],
           o["min_mapping_quality"], o["min_template_length"], o["max_insert_size"], o["paired_end_mode"])
    return np.fromfile(out, dtype=np.float32)


def count_scenario(name, key, contig, start, end, step, read_length=50, length=None, prefill=0, **options):
    counts = reference_count(BAMS[key], contig, start, end, step, read_length, length, prefill, **options)
    arrays[f"c_{name}_counts"] = counts
    meta["count"].append({"name": name, "file": key, "contig": contig, "start": start, "end": end, "step": step,
                          "read_length": read_length, "length": int(counts.size), "prefill": prefill, "options": options})


count_scenario("step50_plain", "main", "chrT", 0, 100000, 50)
count_scenario("step10_plain", "main", "chrT", 0, 100000, 10, flag_exclude=3844, min_mapping_quality=10)
count_scenario("step200_plain", "main", "chrT", 0, 100000, 200, flag_exclude=3844)
count_scenario("step1_pileup", "main", "chrT", 58000, 63000, 1, flag_exclude=3844)
count_scenario("off_grid_region", "main", "chrT", 1237, 98761, 50, flag_exclude=1796)
count_scenario("off_grid_region_step200", "main", "chrT", 33, 77777, 200, min_mapping_quality=30)
count_scenario("single_bin", "main", "chrT", 61000, 61050, 50)
count_scenario("single_bin_wide_step", "main", "chrT", 60990, 61030, 200, extend_bp=150)
count_scenario("extend150", "main", "chrT", 0, 100000, 50, extend_bp=150, flag_exclude=3844, min_mapping_quality=10)
count_scenario("extend1000", "main", "chrT", 0, 100000, 50, extend_bp=1000, flag_exclude=3844)
count_scenario("extend1000_inner_region", "main", "chrT", 20000, 30000, 10, extend_bp=1000)
count_scenario("extend150_contig_head", "main", "chrT", 0, 3000, 1, extend_bp=150, min_mapping_quality=11)
count_scenario("extend150_contig_tail", "main", "chrT", 97000, 100000, 1, extend_bp=150, min_mapping_quality=11)
count_scenario("both_shifts", "main", "chrT", 500, 99500, 50, shift_forward_strand53=4, shift_reverse_strand53=5)
count_scenario("both_shifts_large", "main", "chrT", 20000, 40000, 10, shift_forward_strand53=700, shift_reverse_strand53=-650)
count_scenario("both_shifts_extended", "main", "chrT", 0, 100000, 50, shift_forward_strand53=75, shift_reverse_strand53=75, extend_bp=150)
count_scenario("shift_brings_nothing_in", "main", "chrT", 61100, 62000, 10, shift_forward_strand53=300, shift_reverse_strand53=-300)
count_scenario("one_read_per_bin", "main", "chrT", 0, 100000, 50, one_read_per_bin=1, flag_exclude=3844)
count_scenario("one_read_per_bin_step1", "main", "chrT", 60000, 62000, 1, one_read_per_bin=1)
count_scenario("one_read_per_bin_extended", "main", "chrT", 1237, 98761, 200, one_read_per_bin=1, extend_bp=150)
count_scenario("one_read_per_bin_paired", "main", "chrT", 0, 100000, 50, one_read_per_bin=1, paired_end_mode=1)
count_scenario("paired_default", "main", "chrT", 0, 100000, 50, paired_end_mode=1, flag_exclude=3844)
count_scenario("paired_min_template_set", "main", "chrT", 0, 100000, 50, paired_end_mode=1, min_template_length=200)
count_scenario("paired_min_template_zero", "main", "chrT", 0, 100000, 10, paired_end_mode=1, min_template_length=0)
count_scenario("paired_read_length_fallback", "main", "chrT", 0, 100000, 50, read_length=300, paired_end_mode=1)
count_scenario("paired_no_insert_limit", "main", "chrT", 0, 100000, 50, paired_end_mode=1, max_insert_size=0)
count_scenario("paired_insert500", "main", "chrT", 0, 100000, 50, paired_end_mode=1, max_insert_size=500, min_mapping_quality=10)
count_scenario("paired_shifted", "main", "chrT", 777, 88888, 10, paired_end_mode=1, shift_forward_strand53=4, shift_reverse_strand53=5,
               max_insert_size=500)
count_scenario("flag_include_read1", "main", "chrT", 0, 100000, 50, flag_include=64)
count_scenario("flag_include_pair_bits", "main", "chrT", 0, 100000, 200, flag_include=3, flag_exclude=1024)
count_scenario("into_used_buffer", "main", "chrT", 0, 100000, 50, prefill=7, flag_exclude=3844)
count_scenario("into_used_buffer_one_read", "main", "chrT", 0, 100000, 50, prefill=5, one_read_per_bin=1)
count_scenario("short_buffer", "main", "chrT", 0, 100000, 50, length=1217, extend_bp=150)
count_scenario("short_buffer_one_read", "main", "chrT", 0, 100000, 50, length=1221, one_read_per_bin=1)
count_scenario("empty_contig", "main", "chrE", 0, 30000, 50)
count_scenario("other_contig", "main", "chrU", 0, 40000, 50, flag_exclude=3844)
count_scenario("region_without_reads", "long", "chrL", 500000, 900000, 200)
count_scenario("long_contig_head", "long", "chrL", 0, 450000, 200, extend_bp=150)
count_scenario("big_step50", "big", "chrT", 0, 100000, 50, flag_exclude=3844, min_mapping_quality=10)
count_scenario("big_step10_extended", "big", "chrT", 0, 100000, 10, extend_bp=150, flag_exclude=3844)
count_scenario("big_paired", "big", "chrT", 0, 100000, 50, paired_end_mode=1, flag_exclude=3844, min_mapping_quality=10)
count_scenario("big_one_read_per_bin", "big", "chrT", 123, 99877, 200, one_read_per_bin=1)


def reference_range(bam, contig, chrom_len, flag_exclude):
    a, b = driver("range", bam, contig, chrom_len, flag_exclude).split()
    return int(a), int(b)


for key, contig, chrom_len, flag_exclude in [
        ("main", "chrT", 100000, 3844), ("main", "chrT", 100000, 0), ("main", "chrT", 61020, 3844), ("main", "chrT", 10, 0),
        ("main", "chrE", 30000, 3844), ("main", "chrU", 40000, 3844), ("big", "chrT", 100000, 3844), ("big", "chrT", 100000, 65535),
        ("long", "chrL", 3000000, 3844), ("long", "chrL", 3250000, 0), ("long", "chrL", 5000000, 3844), ("long", "chrL", 2300000, 3844),
        ("long", "chrL", 1250000, 16), ("long", "chrL", 4000, 0), ("noend", "chrN", 2500000, 3844)]:
    start, end = reference_range(BAMS[key], contig, chrom_len, flag_exclude)
    meta["range"].append({"file": key, "contig": contig, "chrom_len": chrom_len, "flag_exclude": flag_exclude, "start": start, "end": end})

# ---- 3. the Python tail: the reference's own get_bam_chrom_reads over a stand-in native module ------------------------
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco")]
sys.modules["rocco"] = pkg
rt = importlib.import_module("rocco.readtracks")
SIZES = os.path.join(WORK, "t.sizes")
with open(SIZES, "w") as handle:
    for name, length in CONTIGS.items():
        handle.write(f"{name}\t{length}\n")
    handle.write("chrX\t1000\n")


class Native:
    """What the whole-file probes would say (prepared), and what the compiled counter says (the driver)."""

    def __init__(self, paired_end, read_length, mapped_reads, fragment_length):
        self.values = dict(paired_end=paired_end, read_length=read_length, mapped_reads=mapped_reads, fragment_length=fragment_length)

    def is_alignment_paired_end(self, *_a, **_k):
        return self.values["paired_end"]

    def get_alignment_read_length(self, *_a, **_k):
        return self.values["read_length"]

    def get_alignment_mapped_read_count(self, *_a, **_k):
        return self.values["mapped_reads"], 0

    def get_alignment_fragment_length(self, *_a, **_k):
        return self.values["fragment_length"]

    def get_alignment_chrom_range(self, bam, chromosome, chrom_size, thread_count=1, flag_exclude=0):
        return reference_range(bam, chromosome, chrom_size, flag_exclude)

    def count_alignment_region(self, bam, chromosome, start, end, step, read_length, thread_count=1, count_mode="coverage", **options):
        assert count_mode == "coverage"
        return reference_count(bam, chromosome, start, end, step, read_length, **options)


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def tail_scenario(name, key, contig, step, native, **kwargs):
    rt._BAM_COUNT_METADATA_CACHE.clear()
    rt._require_native_counter = lambda: native
    keep = Keep()
    rt.logger.addHandler(keep)
    bam = BAMS[key]
    call = dict(effective_genome_size=2.7e9, norm_method="RPGC", min_mapping_score=10, flag_include=None, flag_exclude=3844,
                extend_reads=-1, center_reads=False, ignore_for_norm=None, scale_factor=1.0, num_processors=1, const_scale=1.0,
                round_digits=5, scale_by_step=False)
    call.update(kwargs)
    intervals, vals = rt.get_bam_chrom_reads(bam, contig, SIZES, step, **call)
    metadata = rt._get_bam_count_metadata(bam, step=step, norm_method=call["norm_method"], effective_genome_size=call["effective_genome_size"],
                                          ignore_for_norm=["chrX", "chrY", "chrM"], flag_exclude=call["flag_exclude"],
                                          extend_reads=call["extend_reads"], num_processors=1, scale_factor=call["scale_factor"])
    rt.logger.removeHandler(keep)
    record = {"name": name, "file": key, "contig": contig, "chrom_size": CONTIGS[contig], "step": step, "kwargs": kwargs,
              "native": native.values,
              "metadata": {k: metadata[k] for k in ("read_length", "resolved_extend_bp", "paired_end_mode", "norm_scale")},
              "warnings": [m.replace(bam, "{file}") for m in keep.messages]}
    if intervals is None:
        record["none"] = True
    else:
        arrays[f"t_{name}_intervals"], arrays[f"t_{name}_values"] = np.asarray(intervals), np.asarray(vals)
        record["intervals_dtype"], record["values_dtype"] = str(np.asarray(intervals).dtype), str(np.asarray(vals).dtype)
    meta["tail"].append(record)


single, paired = Native(False, 50, 1234567, 0), Native(True, 50, 2345678, 210)
tail_scenario("rpgc_default", "main", "chrT", 50, single)
tail_scenario("rpkm", "main", "chrT", 50, single, norm_method="RPKM")
tail_scenario("cpm", "main", "chrT", 200, single, norm_method="CPM")
tail_scenario("bpm", "main", "chrT", 10, single, norm_method=" b p m ")
tail_scenario("rpgc_extend150", "main", "chrT", 50, single, extend_reads=150)
tail_scenario("rpgc_inferred_single_end", "main", "chrT", 50, Native(False, 50, 1234567, 180), extend_reads=0)
tail_scenario("rpgc_inference_falls_back", "main", "chrT", 50, Native(False, 50, 1234567, 40), extend_reads=0)
tail_scenario("rpgc_paired_mode", "main", "chrT", 50, paired, extend_reads=0)
tail_scenario("rpgc_paired_without_length", "main", "chrT", 50, Native(True, 50, 2345678, 0), extend_reads=0)
tail_scenario("scale_by_step", "main", "chrT", 50, single, scale_by_step=True)
tail_scenario("scale_by_step_step10", "big", "chrT", 10, single, scale_by_step=True, norm_method="CPM")
tail_scenario("const_scale_third", "main", "chrT", 50, single, const_scale=1.0 / 3.0)
tail_scenario("const_scale_zero", "main", "chrT", 50, single, const_scale=0.0)
tail_scenario("const_scale_negative", "main", "chrT", 50, single, const_scale=-2.0)
tail_scenario("scale_factor", "main", "chrT", 50, single, scale_factor=2.5, norm_method="RPKM")
tail_scenario("round0_half_way", "main", "chrT", 50, Native(False, 50, 2000000, 0), norm_method="CPM", round_digits=0)
tail_scenario("round2_half_way", "main", "chrT", 50, Native(False, 50, 200000000, 0), norm_method="CPM", round_digits=2)
tail_scenario("round5_half_way", "main", "chrT", 50, Native(False, 50, 2000000, 0), norm_method="CPM", scale_factor=1.0e-5, round_digits=5)
tail_scenario("round5_half_way_step10", "big", "chrT", 10, Native(False, 50, 2000000, 0), norm_method="CPM", scale_factor=1.0e-5)
tail_scenario("center_reads", "main", "chrT", 50, single, center_reads=True)
tail_scenario("center_reads_paired", "big", "chrT", 200, paired, center_reads=True, extend_reads=0)
tail_scenario("flag_include", "main", "chrT", 50, single, flag_include=16, min_mapping_score=30)
tail_scenario("keep_everything", "main", "chrT", 50, single, flag_exclude=0, min_mapping_score=0)
tail_scenario("other_contig", "main", "chrU", 50, single)
tail_scenario("big_default", "big", "chrT", 50, single)
tail_scenario("long_contig", "long", "chrL", 200, single)
tail_scenario("start_without_end", "noend", "chrN", 50, single)  # ccounts_getChromRange's asymmetry: (None, None)
tail_scenario("empty_contig", "main", "chrE", 50, single)          # (None, None)
tail_scenario("nothing_passes", "main", "chrT", 50, single, min_mapping_score=300)  # range found, no positive value
tail_scenario("everything_excluded", "main", "chrT", 50, single, flag_exclude=65535)

for norm_method, genome, step, mapped, length, factor in [
        ("RPGC", 2.7e9, 50, 1234567, 50, 1.0), ("rpgc", 2913022398.0, 10, 40000000, 180, 0.5), ("RPGC", 1.0e6, 50, 0, 0, 1.0),
        ("RPKM", -1, 50, 1234567, 50, 1.0), ("RPKM", -1, 200, 7, 36, 3.0), ("CPM", -1, 50, 2000000, 50, 1.0),
        ("BPM", None, 25, 999999, 75, 1.0e-5), ("c p m", -1, 1, 1, 1, 1.0)]:
    meta["scale"].append({"norm_method": norm_method, "effective_genome_size": genome, "step": step, "mapped_reads": mapped,
                          "norm_read_length": length, "scale_factor": factor,
                          "scale": rt._compute_native_scale_factor(norm_method, genome, step, mapped, length, factor)})

np.savez_compressed(os.path.join(HERE, "alignment_count_vectors.npz"), **arrays)
with open(os.path.join(HERE, "alignment_count_vectors.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(meta['count'])} count, {len(meta['range'])} range, {len(meta['tail'])} tail and {len(meta['scale'])} scale scenarios, "
      f"{len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'alignment_count_vectors.npz'))} bytes")
for r in meta["range"]:
    print("  range", r)
for r in meta["tail"]:
    print("  tail ", r["name"], "(None, None)" if r.get("none") else "arrays", r["warnings"])
