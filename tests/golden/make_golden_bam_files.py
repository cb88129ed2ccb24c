#!/usr/bin/env python3
"""BAM files, what htslib decodes from them, and what the REFERENCE's reader returns for them.

    python tests/golden/make_golden_bam_files.py        (by hand, where the reference is mounted; about a minute)

Every stored expectation was written by htslib or by the reference's own Python function:

1. The reference's vendored htslib is built in a temporary directory exactly as make_golden_fragment_length.py builds it
   (settings from the reference's own setup.py).  This project's tests/golden/bam_files_driver.c is linked against it
   (SAM -> BAM, the index, the whole-file dump); fragment_length_driver.c and alignment_counts_driver.c are linked against
   it and the reference's ``native/ccounts_backend.c`` as the stand-in for the reference's compiled counter.  Nothing built
   or copied there is kept.
2. SAM texts made from seeded random arrays become BAM files; the `blocks` file is cut again into BGZF blocks of chosen
   sizes (tests/bam_expected.py: bgzf_compress), so that records and a block_size word straddle block boundaries, and
   htslib reads it back like any other.  The driver dumps tid and the seven values of EVERY record in file order.
3. The NumPy statement of tests/bam_expected.py is held against the dump here already, and the guesses of the record walk
   are checked under its predicate: NO fixture but `decoy` may have a wrong guess at the default segment size (the GPU
   tests demand zero there); `decoy` must have one at DECOY_SEGMENT_BYTES.  Should a seed ever break the first condition,
   change the seed below and say so here.  (Seed 20258: holds.)
4. The reference's own ``get_bam_chrom_reads``, ``_get_bam_count_metadata`` and ``generate_chrom_matrix``
   (rocco/readtracks.py) run with ``_require_native_counter`` replaced IN THE MODULE by a stand-in whose methods call the
   drivers.

Writes tests/golden/bam_files.npz + .json (data only: the BAM files' bytes and the expected arrays)."""
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
WORK = tempfile.mkdtemp(prefix="bam_files_")
DECOY_SEGMENT_BYTES = 4096

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


# ---- 2. SAM texts from seeded random arrays ----------------------------------------------------------------------------
rng = np.random.default_rng(20258)
CONTIGS = [("chrB", 120000), ("chrA", 400000), ("chrC", 90000)]  # (header order is not length order)
CIGARS = [("50M", 50, 50), ("50M", 50, 50), ("50M", 50, 50), ("20M5D30M", 50, 55), ("10S40M", 50, 40), ("25M100N25M", 50, 150),
          ("20M3I27M", 50, 47), ("36M", 36, 36), ("5S30M400N30M5S", 70, 460), ("*", 50, 1), ("30M2P20M", 50, 50), ("25=1X24=", 50, 50),
          ("5H45M", 45, 45)]
BASES = np.array(list("ACGTN"))
arrays, meta = {}, {"files": {}, "decoy_segment_bytes": DECOY_SEGMENT_BYTES, "chrom_reads": [], "metadata": [], "matrix": [], "errors": []}
BAMS = {}


def sequence(n):
    return "".join(BASES[rng.integers(0, 5, size=n)])


def quality(n):
    return "".join(chr(33 + int(q)) for q in rng.integers(0, 42, size=n))


def reads(contig, length, count, prefix="r", seq_rate=0.6):
    """(pos0, line): both strands, pairs of either TLEN sign, mates elsewhere or unmapped, secondary / duplicate records,
    placed-unmapped records, CIGARs with D, N, I, S, H, P, = and X, `*` CIGARs, `*` sequences, qualities present or `*`."""
    lines = []
    for i, pos0 in enumerate(np.sort(rng.integers(0, length - 600, size=count))):
        cigar, qlen, _ = CIGARS[int(rng.integers(0, len(CIGARS)))]
        flag = 16 if rng.random() < 0.5 else 0
        rnext, pnext, tlen = "*", 0, 0
        if rng.random() < 0.5:
            flag |= 1 | (2 if rng.random() < 0.85 else 0) | (64 if rng.random() < 0.5 else 128) | (32 if not flag & 16 else 0)
            tlen = int(rng.integers(20, 900)) * (1 if rng.random() < 0.5 else -1)
            rnext, pnext = ("=" if rng.random() < 0.9 else ("chrC" if contig != "chrC" else "chrA")), int(max(1, pos0 + tlen))
            if rng.random() < 0.04:
                flag |= 8
        flag |= (256 if rng.random() < 0.04 else 0) | (1024 if rng.random() < 0.04 else 0)
        if rng.random() < 0.04:
            flag, cigar = flag | 4, "*"  # unmapped, placed at its mate's position
        mapq = int(rng.integers(0, 61)) if rng.random() < 0.8 else int(rng.choice([0, 9, 10, 11, 255]))
        seq, qual = "*", "*"
        if rng.random() < seq_rate:
            seq = sequence(qlen)
            qual = quality(qlen) if rng.random() < 0.7 else "*"
        name = f"{prefix}{i}" + "x" * int(rng.integers(0, 12))
        lines.append((int(pos0), f"{name}\t{flag}\t{contig}\t{int(pos0) + 1}\t{mapq}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t{seq}\t{qual}"
                      + ("\tNM:i:1\tXS:Z:tag" if rng.random() < 0.3 else "")))
    return lines


def unplaced(count):
    return [f"u{i}\t{4 | (int(rng.integers(0, 2)) * 77 if i % 3 == 0 else 0)}\t*\t0\t0\t*\t*\t0\t0\t{sequence(50) if i % 2 else '*'}\t*" for i in range(count)]


def make_file(key, per_contig, tail=(), cuts_from=None):
    """per_contig: {name: [(pos0, line)]}; tail: lines of records without a contig.  cuts_from(inflated, offsets) -> BGZF cuts."""
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in CONTIGS:
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for name, _ in CONTIGS:
            for _, line in sorted(per_contig.get(name, []), key=lambda item: item[0]):
                handle.write(line + "\n")
        for line in tail:
            handle.write(line + "\n")
    driver("sam2bam", sam, bam)
    if cuts_from is not None:
        with open(bam, "rb") as handle:
            data, _ = bx.inflate(handle.read())
        offsets, _, _, _ = bx.walk(data, bx.header(data)[2])
        with open(bam, "wb") as handle:
            handle.write(bx.bgzf_compress(data, cuts_from(data, offsets)))
    driver("index", bam)
    BAMS[key] = bam
    return bam


def finish_file(key):
    """Stores the file's bytes and htslib's dump; holds the NumPy statement against the dump; returns the inflated bytes."""
    bam = BAMS[key]
    with open(bam, "rb") as handle:
        raw = handle.read()
    out = os.path.join(WORK, key + ".txt")
    driver("dumpall", bam, out)
    with open(out) as handle:
        table = np.asarray(handle.read().split(), dtype=np.int64).reshape(-1, 8)
    arrays[f"bam_{key}"] = np.frombuffer(raw, dtype=np.uint8)
    for column, (field, dtype) in enumerate(bx.FIELDS):
        arrays[f"d_{key}_{field}"] = table[:, column].astype(dtype)
    data, starts = bx.inflate(raw)
    _, contigs, entry0 = bx.header(data)
    assert contigs == CONTIGS
    offsets, end, why, _ = bx.walk(data, entry0)
    assert why == 0 and end == len(data) and offsets.size == table.shape[0], key
    stated, (code, record) = bx.fields(data, offsets, len(contigs))
    cg = key == "cg"
    assert (code == bx.ERR_CG_TAG) if cg else (code == 0), (key, code, record)
    for column, (field, _) in enumerate(bx.FIELDS):
        same = stated[field].astype(np.int64) == table[:, column]
        assert same.all() or (cg and field in ("end", "qlen") and np.flatnonzero(~same).tolist() == [record]), (key, field)
    wrong = bx.wrong_guesses(data, entry0, len(contigs), bx.DEFAULT_SEGMENT_BYTES)
    if wrong and key != "decoy":
        guessed, true = bx.guesses(data, entry0, len(contigs), bx.DEFAULT_SEGMENT_BYTES), bx.true_entries(data, entry0, bx.DEFAULT_SEGMENT_BYTES)
        for i in np.flatnonzero(guessed != true):
            inside = offsets[np.searchsorted(offsets, guessed[i], side="right") - 1]
            print(f"{key}: segment {i} guesses {guessed[i]}, its first record starts at {true[i]}; {guessed[i] - inside} bytes into the "
                  f"record at {inside}: {data[inside: inside + 36].hex()} ... {data[guessed[i]: guessed[i] + 36].hex()}")
        raise SystemExit(f"{key}: {wrong} wrong guesses at the default segment size -- change the seed")
    meta["files"][key] = {"records": int(table.shape[0]), "inflated_bytes": len(data), "bgzf_blocks": len(starts), "first_record": entry0,
                          "wrong_guesses_default": wrong}
    return data, offsets, starts


# the mixed file of row f5's generator, with sequences, qualities and tags, and unplaced reads at the end
make_file("mixed", {"chrB": reads("chrB", 120000, 500), "chrA": reads("chrA", 400000, 900), "chrC": reads("chrC", 90000, 150)}, unplaced(40))


# four BGZF blocks and more: one boundary two bytes into a block_size word, one in the middle of a record's fixed fields
def straddling_cuts(data, offsets):
    third = len(offsets) // 3
    return [int(offsets[third]) + 2, int(offsets[2 * third]) + 17, int(offsets[2 * third + 40]), 3 * len(data) // 4]


make_file("blocks", {"chrB": reads("chrB", 120000, 700, "b"), "chrA": reads("chrA", 400000, 1500, "b")}, unplaced(5), cuts_from=straddling_cuts)
LONG = [(200000, f"long\t0\tchrA\t200001\t40\t1500M20D1500M\t*\t0\t0\t{sequence(3000)}\t{quality(3000)}")]
make_file("longread", {"chrA": reads("chrA", 400000, 300, "s") + LONG, "chrC": reads("chrC", 90000, 60, "s")})
make_file("header_only", {})
make_file("one_record", {"chrA": [(1000, "only\t0\tchrA\t1001\t30\t50M\t*\t0\t0\t*\t*")]})
make_file("unplaced_only", {}, unplaced(30))
# one read of 66 000 CIGAR operations and sequence `*`: htslib keeps its CIGAR in a CG tag and writes `0S66000N` in its place
make_file("cg", {"chrA": reads("chrA", 400000, 20, "c") + [(5000, "many\t0\tchrA\t5001\t30\t" + "1M1D" * 33000 + "\t*\t0\t0\t*\t*")]})


def fake_records(count):
    """`count` well-formed records back to back: 36 fixed bytes and a two-byte name each, on contig 0, no mate."""
    return b"".join(bx.make_record(38, tid=0, pos=1000 + k, name=b"f\0") for k in range(count))


# decoy: a B:C tag holds GUESS_DEPTH + 2 fake records.  Filler records in front of its carrier are added until a segment
# boundary of DECOY_SEGMENT_BYTES falls inside the carrier, in front of the tag: the first fake record is then the lowest
# plausible offset of its segment, and no true record begins there.
FAKE = fake_records(bx.GUESS_DEPTH + 2)
CARRIER = "decoy\t0\tchrA\t300001\t30\t50M\t*\t0\t0\t" + "A" * 50 + "\t*\tXB:B:C," + ",".join(str(b) for b in FAKE)
DECOY_TAIL = reads("chrC", 90000, 80, "e")
for filler in range(200):
    make_file("decoy", {"chrB": reads("chrB", 120000, 40 + filler, "d"), "chrA": [(300000, CARRIER)], "chrC": DECOY_TAIL})
    with open(BAMS["decoy"], "rb") as handle:
        data, _ = bx.inflate(handle.read())
    entry0 = bx.header(data)[2]
    at = data.find(FAKE)
    assert at > 0
    if bx.guesses(data, entry0, len(CONTIGS), DECOY_SEGMENT_BYTES)[at // DECOY_SEGMENT_BYTES] == at and \
            bx.true_entries(data, entry0, DECOY_SEGMENT_BYTES)[at // DECOY_SEGMENT_BYTES] != at:
        meta["decoy_offset"], meta["decoy_filler"] = at, filler
        break
else:
    raise SystemExit("no filler count puts a segment boundary in front of the decoy")

INFLATED = {}
for key in list(BAMS):
    INFLATED[key] = finish_file(key)
data, offsets, starts = INFLATED["blocks"]
assert len(starts) >= 4, "the `blocks` file must span at least three BGZF blocks"
assert any(0 < s - o < 4 for s in starts for o in offsets[np.searchsorted(offsets, s) - 1: np.searchsorted(offsets, s)]), "no block_size word straddles"
data, _, _ = INFLATED["decoy"]
assert bx.plausible_chain(data, meta["decoy_offset"], len(CONTIGS)) and bx.wrong_guesses(data, bx.header(data)[2], len(CONTIGS), DECOY_SEGMENT_BYTES) >= 1

# ---- 4. the reference's own reader over a stand-in native module ---------------------------------------------------------
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
    return result, log


SIZES = os.path.join(WORK, "t.sizes")
with open(SIZES, "w") as handle:
    for name, length in CONTIGS + [("chrZ", 5000)]:  # (chrZ: in the sizes file, not in any header)
        handle.write(f"{name}\t{length}\n")
meta["sizes"] = [[name, length] for name, length in CONTIGS + [("chrZ", 5000)]]

OPTION_SETS = [
    dict(step=50),  # the reference's defaults: RPGC without an effective genome size is its ValueError
    dict(step=50, effective_genome_size=2.7e9, norm_method="RPGC", ignore_for_norm=["chrC"], num_processors=1),
    dict(step=200, norm_method="CPM", min_mapping_score=0, flag_exclude=1796, extend_reads=0, center_reads=True, scale_by_step=True,
         const_scale=2.0, num_processors=1),
    dict(step=100, norm_method="RPKM", extend_reads=150, round_digits=3, flag_include=16, num_processors=2),
]
for key in ("mixed", "blocks", "longread", "one_record", "header_only", "decoy"):
    for contig in [name for name, _ in CONTIGS] + ["chrZ"]:
        for o, options in enumerate(OPTION_SETS):
            options = dict(options)
            step = options.pop("step")
            entry = {"name": f"{key}_{contig}_{o}", "file": key, "contig": contig, "step": step, "kwargs": options, "error": None}
            try:
                (intervals, vals), entry["log"] = logged(lambda: rt.get_bam_chrom_reads(BAMS[key], contig, SIZES, step, **options))
                entry["none"] = intervals is None
                if intervals is not None:
                    arrays[f"r_{entry['name']}_intervals"], arrays[f"r_{entry['name']}_values"] = np.asarray(intervals), np.asarray(vals)
            except (RuntimeError, ValueError) as exc:
                entry["error"], entry["error_type"], entry["log"] = str(exc).replace(SIZES, "{sizes}"), type(exc).__name__, []
            meta["chrom_reads"].append(entry)

for label, call in [("missing_bam", lambda: rt.get_bam_chrom_reads(os.path.join(WORK, "none.bam"), "chrA", SIZES, 50)),
                    ("missing_sizes", lambda: rt.get_bam_chrom_reads(BAMS["mixed"], "chrA", os.path.join(WORK, "none.sizes"), 50)),
                    ("missing_chromosome", lambda: rt.get_bam_chrom_reads(BAMS["mixed"], "chrQ", SIZES, 50))]:
    try:
        call()
        raise SystemExit(f"{label}: the reference raised nothing")
    except (FileNotFoundError, ValueError) as exc:
        text = str(exc).replace(os.path.join(WORK, "none.bam"), "{bam}").replace(os.path.join(WORK, "none.sizes"), "{sizes}").replace(SIZES, "{sizes}")
        meta["errors"].append({"label": label, "type": type(exc).__name__, "message": text})

for key in ("mixed", "blocks", "longread", "one_record"):
    for call in (dict(step=50, norm_method="RPGC", effective_genome_size=2.7e9, ignore_for_norm=None, num_processors=3),
                 dict(step=200, norm_method="c p m", effective_genome_size=None, ignore_for_norm=["chrB"], flag_exclude=3844, extend_reads=0,
                      num_processors=1, scale_factor=2.5)):
        metadata, log = logged(lambda: rt._get_bam_count_metadata(BAMS[key], **call))
        meta["metadata"].append({"file": key, "call": call, "metadata": metadata, "log": log})

MATRIX_FILES = ["mixed", "blocks", "longread"]
for contig, options in (("chrA", dict(step=50, num_processors=1, effective_genome_size=2.7e9)), ("chrC", dict(step=100, num_processors=1, norm_method="CPM", extend_reads=150)),
                        ("chrB", dict(step=50, num_processors=1, effective_genome_size=1.0e6, low_memory=True))):
    options = dict(options)
    step = options.pop("step")
    (intervals, matrix), log = logged(lambda: rt.generate_chrom_matrix(contig, [BAMS[k] for k in MATRIX_FILES], SIZES, step, **options))
    name = f"m_{contig}"
    arrays[f"{name}_intervals"], arrays[f"{name}_matrix"] = np.asarray(intervals), np.asarray(matrix)
    meta["matrix"].append({"name": name, "contig": contig, "files": MATRIX_FILES, "step": step, "kwargs": options, "log": log})

np.savez_compressed(os.path.join(HERE, "bam_files.npz"), **arrays)
with open(os.path.join(HERE, "bam_files.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(BAMS)} files, {len(meta['chrom_reads'])} chrom_reads, {len(meta['metadata'])} metadata and {len(meta['matrix'])} matrix scenarios, "
      f"{len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'bam_files.npz'))} bytes")
for key, facts in meta["files"].items():
    print("  ", key, facts)
print("   decoy at", meta["decoy_offset"], "after", meta["decoy_filler"], "fillers")
