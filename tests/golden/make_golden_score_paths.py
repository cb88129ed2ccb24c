#!/usr/bin/env python3
"""What the REFERENCE makes of BAM PATHS in its post-hoc scoring and in its narrowPeak step.

    make -C oracle ref
    python tests/golden/make_golden_score_paths.py        (by hand, where the reference is mounted; a few minutes)

1. The reference's vendored htslib and its counter are built as make_golden_interval_counts.py builds them; this project's
   three drivers (alignment_counts_driver.c, bam_files_driver.c, bam_index_driver.c, unchanged) are linked against them.
2. Three coordinate-sorted BAM files over five contigs (one without records) from seeded SAM text, written and indexed by
   htslib.  Stored: the BAM bytes, the ``.bai`` bytes, htslib's dump of every record and, per contig, the index
   statistics and the ordinals of the records the index iterator yields.
3. A stand-in ``pysam`` module made of those dumps alone: ``.mapped`` (the sum of ``hts_idx_get_stat``'s mapped counts),
   ``.count(contig)`` (the number of iterator ordinals; ValueError for an unknown contig), ``.count(contig, start, stop,
   read_callback)`` (the driver at the null's options, as in make_golden_interval_counts.py), ``.fetch()`` (the header's
   contigs one behind the other, each in iterator order; ``infer_query_length()`` is None for a query length of 0).
   pysam itself is not installed: DESIGN.md note (33) says what that leaves argued.
4. The reference's own ``get_read_length``, ``raw_count_matrix``, ``get_ecdf``, ``multi_ecdf``, ``score_peaks``
   (rocco/scores.py) and ``_generate_narrowpeak_if_requested`` (rocco/rocco.py) run as they are, with ``_hts_counts``
   replaced in the module by the driver; their files, return values, exception types and log records are stored.

Writes tests/golden/score_paths.npz + .json (data only)."""
import importlib
import json
import logging
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
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="score_paths_")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_index_files as bif  # noqa: E402  (the older fixtures' bytes)

# ---- 1. htslib, the counter, the drivers ---------------------------------------------------------------------------------
HTS = os.path.join(WORK, "htslib")
shutil.copytree(os.path.join(REFERENCE, "vendor", "htslib"), HTS)


def reference_build_settings():
    """The module-level assignments and functions of the reference's setup.py (importing it would run ``setup()``)."""
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
NATIVE = os.path.join(REFERENCE, "rocco", "native")
BINARIES = {}
for binary, sources in (("count", ["alignment_counts_driver.c", os.path.join(NATIVE, "ccounts_backend.c")]),
                        ("files", ["bam_files_driver.c"]), ("index", ["bam_index_driver.c"])):
    BINARIES[binary] = os.path.join(WORK, binary + "_driver")
    subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS, "-I", NATIVE, *[os.path.join(HERE, s) for s in sources],
                    os.path.join(HTS, "libhts.a"), "-lz", "-lm", "-lpthread", "-o", BINARIES[binary]], check=True)


def driver(*args, binary="files"):
    return subprocess.run([BINARIES[binary], *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout


# ---- 2. the files --------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(20331)
CONTIGS = [("chr1", 50000), ("chrX", 20000), ("chr2", 120000), ("chrY", 30000), ("chrM", 40000)]  # chrX: no records; the names
# are those of the reference's default ``skip_for_norm``, which its narrowPeak step cannot change
CIGARS = ["50M", "50M", "50M", "20M5D30M", "10S40M", "25M100N25M", "20M3I27M", "36M", "5S30M400N30M5S", "75M", "101M"]
PILE = 61000
FILES = ["p1", "p2", "p3"]
arrays, meta = {}, {"contigs": CONTIGS, "files": {}, "pile_position": PILE}


def sam_lines(contig, positions, prefix, low_mapq=0.2):
    """Both strands, pairs, secondary and supplementary records, placed-unmapped mates (no CIGAR), mapping qualities over
    0 .. 60; every mapped record has a CIGAR."""
    lines = []
    for i, p in enumerate(positions):
        cigar = CIGARS[int(rng.integers(0, len(CIGARS)))]
        flag = 16 if rng.random() < 0.5 else 0
        rnext, pnext, tlen = "*", 0, 0
        if rng.random() < 0.5:
            flag |= 1 | (2 if rng.random() < 0.85 else 0) | (64 if rng.random() < 0.5 else 128)
            tlen = int(rng.integers(20, 900)) * (1 if rng.random() < 0.5 else -1)
            rnext, pnext = "=", int(max(1, p + tlen))
        flag |= 256 if rng.random() < 0.04 else 0
        flag |= 2048 if rng.random() < 0.03 else 0
        if rng.random() < 0.03:
            flag, cigar = (flag | 4 | 1) & ~(2 | 256 | 2048), "*"  # an unmapped mate, placed at its mate's position
        mapq = int(rng.integers(0, 10)) if rng.random() < low_mapq else int(rng.integers(10, 61))
        lines.append(f"{prefix}{i}\t{flag}\t{contig}\t{int(p) + 1}\t{mapq}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t*\t*")
    return lines


def spread(size, n, pile=0):
    pos = rng.integers(200, size - 1000, size=n)
    return np.sort(np.concatenate([pos, np.full(pile, PILE, dtype=np.int64)]), kind="stable")


def dump_file(key, bam):
    """htslib's view of a file that lies in WORK with its index: the records, and per contig statistics and ordinals."""
    out = os.path.join(WORK, key + ".all.txt")
    driver("dumpall", bam, out)
    table = np.loadtxt(out, dtype=np.int64, ndmin=2).reshape(-1, 8)
    arrays[f"rec_{key}"] = table.astype(np.int32)  # tid pos end isize flag mapq mate_same qlen, file order
    out = os.path.join(WORK, key + ".idx.txt")
    driver("dump", bam, out, binary="index")
    entry = {"refs": [], "records": int(table.shape[0])}
    with open(out) as handle:
        for line in handle:
            words = line.split()
            if words[0] == "ref":
                t, has_stat, mapped, unmapped, n = (int(w) for w in words[1:6])
                arrays[f"itr_{key}_{t}"] = np.asarray(words[6:], dtype=np.int64)
                entry["refs"].append({"has_stat": bool(has_stat), "mapped": mapped, "unmapped": unmapped, "records": n})
            elif words[0] == "nocoor":
                entry["n_no_coor"] = int(words[1])
    meta["files"][key] = entry
    return entry


def make_file(key, per_contig, tail, low_mapq):
    sam, bam = os.path.join(WORK, key + ".sam"), os.path.join(WORK, key + ".bam")
    with open(sam, "w") as handle:
        handle.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, length in CONTIGS:
            handle.write(f"@SQ\tSN:{name}\tLN:{length}\n")
        for name, _ in CONTIGS:
            if name in per_contig:
                for line in sam_lines(name, per_contig[name], name[-1].lower(), low_mapq):
                    handle.write(line + "\n")
        for i in range(tail):
            handle.write(f"u{i}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n")
    driver("sam2bam", sam, bam)
    driver("index", bam)
    for suffix, name in ((".bam", "bam"), (".bam.bai", "bai")):
        with open(os.path.join(WORK, key + suffix), "rb") as handle:
            arrays[f"{name}_{key}"] = np.frombuffer(handle.read(), dtype=np.uint8)
    dump_file(key, bam)
    return bam


BAMS = {
    "p1": make_file("p1", {"chr1": spread(50000, 1700), "chr2": spread(120000, 500, pile=650), "chrY": spread(30000, 80),
                           "chrM": spread(40000, 90)}, 20, 0.2),
    "p2": make_file("p2", {"chr1": spread(50000, 450), "chr2": spread(120000, 600), "chrY": spread(30000, 60),
                           "chrM": spread(40000, 90)}, 9, 0.04),
    "p3": make_file("p3", {"chr1": spread(50000, 150), "chr2": spread(120000, 180), "chrM": spread(40000, 70)}, 5, 0.2),
}
OLD = ["header_only", "unplaced_only", "wide"]
for key in OLD:
    BAMS[key] = bif.write_indexed(WORK, key)
    dump_file(key, BAMS[key])
KEY_OF = {path: key for key, path in BAMS.items()}
NAMES = {key: [name for name, _ in CONTIGS] for key in FILES}
for key in OLD:  # (their headers: read back from the fixture the index tests use)
    NAMES[key] = [name for name, _ in bif.golden()[1]["files"][key]["contigs"]]
largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE))
assert all(arrays[f"bam_{k}"].size <= largest for k in FILES)


# ---- 3. the stand-in pysam -----------------------------------------------------------------------------------------------
class Read:
    def __init__(self, row):
        flag = int(row[4])
        self.is_unmapped, self.is_secondary, self.is_supplementary = bool(flag & 4), bool(flag & 256), bool(flag & 2048)
        self.mapping_quality, self._qlen = int(row[5]), int(row[7])

    def infer_query_length(self):
        return self._qlen if self._qlen != 0 else None


DEFAULTS = dict(one_read_per_bin=0, flag_include=0, flag_exclude=0, shift_forward_strand53=0, shift_reverse_strand53=0,
                extend_bp=0, max_insert_size=1000, paired_end_mode=0, min_mapping_quality=0, min_template_length=-1, read_length=0)
NULL_OPTIONS = dict(one_read_per_bin=1, flag_exclude=4, min_mapping_quality=10)
_tls = threading.local()


def interval_count(bam, contig, start, end, **options):
    """One interval of count_alignment_intervals: region [start, end), intervalSizeBP = end - start, a buffer of one float."""
    o = dict(DEFAULTS, **options)
    if getattr(_tls, "pid", None) != os.getpid():  # (multi_ecdf forks: one output file per process and thread)
        _tls.pid, _tls.out = os.getpid(), os.path.join(WORK, f"count_{os.getpid()}_{threading.get_ident()}.f32")
    driver("count", bam, contig, start, end, end - start, 1, 0, _tls.out, o["one_read_per_bin"], o["flag_include"],
           o["flag_exclude"], o["shift_forward_strand53"], o["shift_reverse_strand53"], o["read_length"], o["extend_bp"],
           o["min_mapping_quality"], o["min_template_length"], o["max_insert_size"], o["paired_end_mode"], binary="count")
    return float(np.fromfile(_tls.out, dtype=np.float32)[0])


class AlignmentFile:
    """pysam.AlignmentFile as rocco/scores.py uses it, from htslib's dumps."""

    def __init__(self, path, mode="rb", threads=1):
        self.path, self.key = path, KEY_OF[path]
        self.mapped = sum(ref["mapped"] for ref in meta["files"][self.key]["refs"])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def close(self):
        pass

    def count(self, contig=None, start=None, stop=None, read_callback=None):
        if contig not in NAMES[self.key]:
            raise ValueError(f"invalid contig `{contig}`")
        if start is None:
            return int(arrays[f"itr_{self.key}_{NAMES[self.key].index(contig)}"].size)
        # _check_read: mapped and mapping_quality >= 10, over what the index iterator yields
        return int(interval_count(self.path, contig, int(start), int(stop), **NULL_OPTIONS))

    def fetch(self):
        table = arrays[f"rec_{self.key}"]
        for t in range(len(NAMES[self.key])):
            for ordinal in arrays[f"itr_{self.key}_{t}"]:
                yield Read(table[int(ordinal)])


pysam = types.ModuleType("pysam")
pysam.AlignmentFile = AlignmentFile
pysam.AlignedSegment = object
sys.modules["pysam"] = pysam
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco"), os.path.join(ROOT, "oracle", "_ref")]
sys.modules["rocco"] = pkg
sc = importlib.import_module("rocco.scores")
impl = importlib.import_module("rocco.rocco")
POOL = ThreadPoolExecutor(16)


class Native:
    def count_alignment_intervals(self, bam, chroms, starts, ends, thread_count=1, count_mode="coverage", **options):
        assert count_mode == "coverage"
        return np.asarray(list(POOL.map(lambda a: interval_count(bam, a[0], int(a[1]), int(a[2]), **options), zip(chroms, starts, ends))),
                          dtype=np.float32)


sc._hts_counts = Native()

# log records: (level, message) with WORK written as {dir}; the handler writes through one O_APPEND descriptor, so that
# the records of multi_ecdf's forked workers (proc = 1: one worker, in order) arrive too
LOG = os.path.join(WORK, "log.jsonl")
LOG_FD = os.open(LOG, os.O_WRONLY | os.O_CREAT | os.O_APPEND)


class Keep(logging.Handler):
    def emit(self, record):
        os.write(LOG_FD, (json.dumps([record.levelname, record.getMessage().replace(WORK, "{dir}")]) + "\n").encode())


for name in ("rocco.scores", "rocco.rocco"):
    logging.getLogger(name).addHandler(Keep())
    logging.getLogger(name).setLevel(logging.INFO)


def logged(call):
    """(what `call` returns or the exception it raises, the log records it left)"""
    before = os.path.getsize(LOG)
    try:
        result, error = call(), None
    except Exception as exc:  # noqa: BLE001  (the type is what is recorded)
        result, error = None, exc
    with open(LOG) as handle:
        handle.seek(before)
        records = [json.loads(line) for line in handle]
    return result, error, records


def file_bytes(path):
    with open(path, "rb") as handle:
        return np.frombuffer(handle.read(), dtype=np.uint8)


# ---- 4a. get_read_length ---------------------------------------------------------------------------------------------------
def qualifying(key, min_mapq):
    """Per contig (header order): the rows fetch() yields and which of them qualify."""
    table = arrays[f"rec_{key}"]
    out = []
    for t in range(len(NAMES[key])):
        rows = table[arrays[f"itr_{key}_{t}"]]
        out.append((rows, ((rows[:, 4] & (4 | 256 | 2048)) == 0) & (rows[:, 5] >= min_mapq)))
    return out


meta["read_length"], census = [], {}
for key in FILES + OLD:
    for num_reads, min_mapq in ((1000, 10), (50, 10), (50, 30)):
        value, error, _ = logged(lambda: sc.get_read_length(BAMS[key], num_reads, min_mapq))
        meta["read_length"].append({"file": key, "num_reads": num_reads, "min_mapping_quality": min_mapq,
                                    "value": value, "error": type(error).__name__ if error is not None else None})
for key in FILES:  # where the quota of 1000 / of 50 is filled
    per_contig = qualifying(key, 10)
    sizes = [int(np.count_nonzero(q)) for _, q in per_contig]
    nonempty = [t for t, (rows, _) in enumerate(per_contig) if rows.shape[0] > 0]
    census[key] = {"qualifying_per_contig": sizes, "fills_1000_in_first_contig": sizes[nonempty[0]] >= 1000,
                   "runs_out": sum(sizes) < 1000, "fills_50_inside_first_contig": sizes[nonempty[0]] > 50}
    rows, q = per_contig[nonempty[0]]
    cut = int(np.flatnonzero(q)[49])  # the window of the first 50 qualifying records
    window = rows[:cut + 1]
    census[key]["rejected_in_window_of_50"] = {
        "unmapped": int(np.count_nonzero(window[:, 4] & 4)), "secondary": int(np.count_nonzero(window[:, 4] & 256)),
        "supplementary": int(np.count_nonzero(window[:, 4] & 2048)), "low_mapq": int(np.count_nonzero(window[:, 5] < 10))}
meta["census"] = census
assert census["p1"]["fills_1000_in_first_contig"] and census["p3"]["runs_out"], census
assert not census["p2"]["fills_1000_in_first_contig"] and not census["p2"]["runs_out"], census
assert all(census[k]["fills_50_inside_first_contig"] for k in FILES), census
assert any(all(v > 0 for v in census[k]["rejected_in_window_of_50"].values()) for k in FILES), census
assert all(r["value"] is not None for r in meta["read_length"] if r["file"] in FILES)
pile = arrays["rec_p1"]
assert int(np.count_nonzero((pile[:, 0] == 2) & (pile[:, 1] == PILE))) >= 600
for key in FILES:
    mapped_rows = arrays[f"rec_{key}"][(arrays[f"rec_{key}"][:, 4] & 4) == 0]
    assert np.all(mapped_rows[:, 7] > 0), "a mapped record without a CIGAR"

# ---- 4b. the counting functions ---------------------------------------------------------------------------------------------
SIZES = os.path.join(WORK, "g.sizes")
with open(SIZES, "w") as handle:
    for name, length in CONTIGS:
        handle.write(f"{name}\t{length}\n")
meta["sizes_text"] = open(SIZES).read()
SIZE_OF = dict(CONTIGS)
peak_rows = []
for _ in range(60):
    contig = str(rng.choice(["chr2", "chr2", "chr1", "chr1", "chrM", "chrY"]))
    length = int(rng.integers(150, 2500))
    start = int(rng.integers(0, SIZE_OF[contig] - length))
    peak_rows.append((contig, start, start + length))
peak_rows += [("chr2", PILE - 300, PILE + 400), ("chr2", PILE, PILE + 180), ("chrX", 5000, 5600), ("chr1", 100, 700)]
order = {name: k for k, (name, _) in enumerate(CONTIGS)}
peak_rows.sort(key=lambda r: (-order[r[0]], r[1]))  # (not the header's order)
PEAKS = os.path.join(WORK, "peaks.bed")
with open(PEAKS, "w") as handle:
    for row in peak_rows:
        handle.write("\t".join(str(v) for v in row) + "\n")
meta["peaks_text"] = open(PEAKS).read()
BAM_LIST = [BAMS[k] for k in FILES]
meta["sample_names"] = FILES

TSV = os.path.join(WORK, "raw.counts.tsv")
_, error, records = logged(lambda: sc.raw_count_matrix(BAM_LIST, PEAKS, TSV, bed_columns=3))
assert error is None
arrays["raw_count_matrix_tsv"] = file_bytes(TSV)
meta["raw_count_matrix_log"] = records
_, error, records = logged(lambda: sc.raw_count_matrix(BAM_LIST, PEAKS, TSV, bed_columns=3))  # (the file exists: the warning)
assert error is None and arrays["raw_count_matrix_tsv"].tobytes() == file_bytes(TSV).tobytes()
meta["raw_count_matrix_again_log"] = records

meta["get_ecdf"] = []
for label, kwargs in [("plain", dict(length=400, nsamples=40, sample_scaling_constants=None, seed=5)),
                      ("scaled_trimmed", dict(length=1500, nsamples=50, sample_scaling_constants=[2.5, 11.25, 30.5], seed=9,
                                              trim_proportion=0.1, row_scale=500.0, pc=0.5))]:
    null, error, records = logged(lambda: sc.get_ecdf(BAM_LIST, chrom_sizes_file=SIZES, **kwargs))
    assert error is None
    arrays[f"ecdf_{label}_values"] = null.values
    meta["get_ecdf"].append({"name": label, "kwargs": kwargs, "log": records})

multi_kwargs = dict(lengths=[300, 900, 300, 2000], nsamples_per_length=25, sample_scaling_constants=[1.5, 4.0, 9.0], seed=21,
                    row_scale=1000.0, pc=1.0)
nulls, error, records = logged(lambda: sc.multi_ecdf(BAM_LIST, chrom_sizes_file=SIZES, proc=1, **multi_kwargs))
assert error is None
arrays["multi_ecdf_lengths"] = np.asarray(list(nulls), dtype=np.int64)
for length, null in nulls.items():
    arrays[f"multi_ecdf_{int(length)}"] = null.values
meta["multi_ecdf"] = {"kwargs": multi_kwargs, "log": records}

SUMMITS = os.path.join(WORK, "summits.tsv")
names = ["_".join(str(v) for v in row) for row in peak_rows]
with open(SUMMITS, "w") as handle:
    handle.write(f"{names[0]}\t17\n{names[5]}\t999999\n\n{names[9]}\t0\n")
meta["summit_offsets_text"] = open(SUMMITS).read()
meta["score_peaks"] = []
score_cases = [
    ("no_matrix", dict(skip_for_norm=["chrX"], ecdf_nsamples=30, ecdf_max_length_bins=4, seed=77), False),
    ("existing_matrix", dict(skip_for_norm=["chrX"], ecdf_nsamples=30, ecdf_max_length_bins=4, seed=77), True),
    ("skip_with_records", dict(skip_for_norm=["chrY", "chrX"], ecdf_nsamples=20, ecdf_max_length_bins=3, seed=5, row_scale=500, pc=2,
                               ucsc_base=100), False),
]
for label, kwargs, keep_matrix in score_cases:
    matrix = os.path.join(WORK, f"{label}.counts.tsv")
    scored = os.path.join(WORK, f"{label}.narrowPeak")
    if keep_matrix:
        shutil.copy(os.path.join(WORK, "no_matrix.counts.tsv"), matrix)
    result, error, records = logged(lambda: sc.score_peaks(BAM_LIST, chrom_sizes_file=SIZES, peak_file=PEAKS, count_matrix_file=matrix,
                                                           output_file=scored, threads=1, proc=1, summit_offsets_file=SUMMITS, **kwargs))
    entry = {"name": label, "kwargs": kwargs, "existing_matrix": keep_matrix, "log": records,
             "error": type(error).__name__ if error is not None else None}
    if error is None:
        arrays[f"score_{label}_narrowpeak"], arrays[f"score_{label}_tsv"] = file_bytes(scored), file_bytes(matrix)
        arrays[f"score_{label}_scores"], arrays[f"score_{label}_bed6"], arrays[f"score_{label}_pvals"] = (
            result[0], np.asarray(result[1]), result[2])
    meta["score_peaks"].append(entry)
assert [e["error"] for e in meta["score_peaks"]] == [None, None, None], meta["score_peaks"]
# a contig of skip_for_norm that the header does not have: `wide` (chrB .. chrC), chrM
WIDE_SIZES, WIDE_PEAKS = os.path.join(WORK, "wide.sizes"), os.path.join(WORK, "wide.bed")
wide_contigs = bif.golden()[1]["files"]["wide"]["contigs"]
with open(WIDE_SIZES, "w") as handle:
    handle.write("".join(f"{name}\t{length}\n" for name, length in wide_contigs))
with open(WIDE_PEAKS, "w") as handle:
    handle.write("chrB\t1000\t1800\nchrB\t60000\t60400\nchrA\t5000\t7000\n")
_, error, _ = logged(lambda: sc.score_peaks([BAMS["wide"]], chrom_sizes_file=WIDE_SIZES, peak_file=WIDE_PEAKS,
                                            count_matrix_file=os.path.join(WORK, "wide.counts.tsv"),
                                            output_file=os.path.join(WORK, "wide.narrowPeak"), skip_for_norm=["chrM"],
                                            ecdf_nsamples=5, seed=3, threads=1, proc=1))
meta["skip_absent"] = {"file": "wide", "sizes_text": open(WIDE_SIZES).read(), "peaks_text": open(WIDE_PEAKS).read(),
                       "skip_for_norm": ["chrM"], "error": type(error).__name__ if error is not None else None}
assert meta["skip_absent"]["error"] == "ValueError", error
assert arrays["score_no_matrix_narrowpeak"].tobytes() == arrays["score_existing_matrix_narrowpeak"].tobytes()
meta["mapped"] = {k: sum(ref["mapped"] for ref in meta["files"][k]["refs"]) for k in FILES}

# ---- 4c. the narrowPeak step ------------------------------------------------------------------------------------------------
small = [("chr1", 1000, 1600), ("chr1", 20000, 21500), ("chr2", PILE - 200, PILE + 300), ("chr2", 90000, 90400), ("chrM", 3000, 3900)]
meta["narrowpeak_bed_text"] = "".join("\t".join(str(v) for v in row) + "\n" for row in small)
tracks = {}
for contig in ("chr1", "chr2"):  # (chrM has no summit track: its peak gets -1)
    edges = np.arange(0, SIZE_OF[contig] + 1, 50, dtype=np.int64)
    tracks[contig] = (edges, rng.normal(size=edges.size - 1).astype(np.float32))
    arrays[f"np_track_{contig}_intervals"], arrays[f"np_track_{contig}_mean"] = tracks[contig]
meta["narrowpeak"] = []
np_cases = [("ends_bed", "out_a.bed", "bam", BAM_LIST), ("ends_BED", "out_b.BED", "bam", BAM_LIST), ("no_extension", "out_c", "bam", BAM_LIST),
            ("bigwig", "out_d.bed", "bigwig", BAM_LIST), ("failing", "out_e.bed", "bam", BAM_LIST + [os.path.join(WORK, "missing.bam")])]
for label, output, track_type, inputs in np_cases:
    folder = os.path.join(WORK, "np_" + label)
    os.mkdir(folder)
    final_output = os.path.join(folder, output)
    with open(final_output, "w") as handle:
        handle.write(meta["narrowpeak_bed_text"])
    cache = {contig: {"summit_track_file": impl._cpy_narrowpeak_summit_track(contig, *tracks[contig])} for contig in tracks}
    args = {"narrowPeak": True, "input_track_type": track_type, "input_files": inputs, "chrom_sizes_file": SIZES, "ecdf_samples": 25,
            "ecdf_seed": 13, "ecdf_proc": 1}
    _, error, records = logged(lambda: impl._generate_narrowpeak_if_requested(args, final_output, cache))
    assert error is None
    entry = {"name": label, "output": output, "input_track_type": track_type, "log": records, "missing_input": label == "failing",
             "files": sorted(f for f in os.listdir(folder) if f != output)}
    for produced in entry["files"]:
        arrays[f"np_{label}_{produced}"] = file_bytes(os.path.join(folder, produced))
    meta["narrowpeak"].append(entry)
    for contig in cache:
        os.remove(cache[contig]["summit_track_file"])
assert [len(e["files"]) for e in meta["narrowpeak"]] == [2, 2, 2, 0, 0], meta["narrowpeak"]
assert not [f for f in os.listdir(tempfile.gettempdir()) if f.startswith("rocco_pointsource_")], "an offsets file was left behind"

np.savez_compressed(os.path.join(HERE, "score_paths.npz"), **arrays)
with open(os.path.join(HERE, "score_paths.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
size = os.path.getsize(os.path.join(HERE, "score_paths.npz"))
assert size < (1 << 20), size
shutil.rmtree(WORK)
print(f"wrote {len(arrays)} arrays, {size} bytes; census {json.dumps(census)}")
