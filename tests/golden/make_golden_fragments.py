#!/usr/bin/env python3
"""What the REFERENCE makes of fragments files.

    python tests/golden/make_golden_fragments.py        (by hand, where the reference is mounted; about a minute)

Every stored result was written by the reference's compiled C:

1. The reference's vendored htslib is copied into a temporary directory and built as make_golden_alignment_counts.py builds
   it; the reference's ``native/ccounts_backend.c`` is compiled against it together with this project's driver
   (tests/golden/fragments_driver.c).  Nothing built or copied there is kept.
2. Texts made from seeded random arrays become BGZF files with a ``.tbi`` (the driver's ``pack``: htslib's ``bgzf_write`` and
   ``tbx_index_build`` with ``tbx_conf_bed``); the driver dumps the lines the index iterator yields per contig (``dump``) and
   calls ``ccounts_getChromRange`` (``range``), ``ccounts_openSource`` / ``ccounts_countRegion`` (``count``),
   ``ccounts_getMappedReadCount`` (``mapped``) and ``ccounts_getReadLength`` (``readlen``), each with
   ``sourceKind = ccounts_sourceKindFragments``, with and without an allow-list.
3. The reference's own ``get_bam_chrom_reads`` and ``_get_bam_count_metadata`` (rocco/readtracks.py:242-353, 389-518) run
   with ``_require_native_counter`` replaced IN THE MODULE by a stand-in that forwards every call to the driver with the
   fragments source kind, the scenario's allow-list and the scenario's count mode: (intervals, values), metadata dicts, log
   records, (None, None) cases and exceptions are stored.
4. A census (tests/fragments_expected.py replays every call and says which rule every line met) asserts that every skip
   rule is hit at least once per consumer and that every mode reaches both of its branches.

htslib refuses to index a line whose end lies below its begin (hts_idx_push: "Invalid record"), so ``end < start`` stands only
in the file without an index that the read-length probe reads.

Writes tests/golden/fragments.npz + .json (data only: the bytes of every .tsv.gz, .tbi and allow-list, and every result)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fragments_expected as fx  # noqa: E402

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="fragments_")

# ---- 1. the reference's counter -------------------------------------------------------------------------------------
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
subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS, "-I", os.path.join(REFERENCE, "rocco", "native"),
                os.path.join(HERE, "fragments_driver.c"), os.path.join(REFERENCE, "rocco", "native", "ccounts_backend.c"),
                os.path.join(HTS, "libhts.a"), "-lz", "-lm", "-lpthread", "-o", DRIVER], check=True)


def driver(*args):
    return subprocess.run([DRIVER, *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout.strip()


# ---- 2. texts from seeded random arrays --------------------------------------------------------------------------------
rng = np.random.default_rng(20261)
SIZES = {"chrA": 200000, "chrB": 60000, "chrC": 50000, "chrE": 30000}  # (chrD is in the files, not in the sizes file)
BARCODES = [("".join(rng.choice(list("ACGT"), size=16)) + "-1").encode() for _ in range(400)]
LONG_BARCODE = b"ACGT" * 1250  # 5 000 bytes
arrays, meta = {}, {"files": {}, "allowlists": {}, "dump": [], "range": [], "count": [], "mapped": [], "readlen": [], "sizes": SIZES}


def plain_lines(contig, n, lo, hi, fields=5):
    starts = np.sort(rng.integers(lo, hi, size=n))
    out = []
    for s in starts:
        e = int(s) + int(rng.integers(20, 600))
        parts = [contig.encode(), str(int(s)).encode(), str(e).encode(), BARCODES[int(rng.integers(0, len(BARCODES)))],
                 str(int(rng.integers(1, 6))).encode()]
        out.append((int(s), b"\t".join(parts[:fields])))
    return out


def odd_lines(contig, lo, hi):
    """One line (or a few) per trap of the issue, at seeded places."""
    c = contig.encode()
    bc = BARCODES[3]
    out = []

    def at():
        return int(rng.integers(lo, hi))

    for tail in (b"", b"\t" + bc, b"\t" + bc + b"\t2", b"\t" + bc + b"\t2\tx\ty",          # 3, 4, 5 and 7 fields
                 b"\t" + bc + b"\t3\t",                                                   # a trailing tab
                 b"\t",                                                                   # ... behind three fields
                 b"\t\t4",                                                                # an empty barcode
                 b"\t" + bc + b"\t",                                                      # an empty fifth field
                 b"\t\t",                                                                 # the last field scanned is empty
                 b"\t" + bc + b"\t0", b"\t" + bc + b"\t-2", b"\t" + bc + b"\tx", b"\t" + bc + b"\t12x",
                 b"\t" + LONG_BARCODE + b"\t2",
                 b"\t" + BARCODES[5] + b"\t1\r", b"\t" + BARCODES[6] + b"\r", b"\r",       # CRLF endings
                 b"\t" + BARCODES[7][:9] + b"\t1",                                        # a proper prefix of an allowed barcode
                 b"\t" + BARCODES[8] + b"X\t1"):                                          # an allowed barcode is its proper prefix
        for _ in range(3):
            s = at()
            out.append((s, c + b"\t%d\t%d" % (s, s + int(rng.integers(20, 600))) + tail))
    for _ in range(3):
        s = at()
        out.append((s, c + b"\t%d\t%d\t" % (s, s) + bc + b"\t1"))                           # end == start
    return out


def text_of(per_contig, header=(b"# a header line", b"#chrA\t1\t2\tnot-a-fragment\t9"), inner_meta=True, terminated=True):
    lines = list(header)
    for contig, entries in per_contig:
        entries = sorted(entries, key=lambda e: e[0])
        body = [e[1] for e in entries]
        if inner_meta and len(body) > 4:
            body.insert(len(body) // 2, b"# a meta line between two lines of " + contig.encode())
        lines += body
    text = b"".join(line + b"\n" for line in lines)
    return text if terminated else text[:-1]


def make_file(key, text, cuts=()):
    txt, gz = os.path.join(WORK, key + ".tsv"), os.path.join(WORK, key + ".tsv.gz")
    with open(txt, "wb") as handle:
        handle.write(text)
    driver("pack", txt, gz, *cuts)
    arrays[f"file_{key}_gz"] = np.fromfile(gz, dtype=np.uint8)
    arrays[f"file_{key}_tbi"] = np.fromfile(gz + ".tbi", dtype=np.uint8)
    contigs = []
    for line in fx.split_lines(text):
        name = line.split(b"\t")[0].decode()
        if not line.startswith(b"#") and name not in contigs:
            contigs.append(name)
    meta["files"][key] = {"contigs": contigs, "cuts": [int(c) for c in cuts]}
    for contig in contigs + ["chrNone"]:
        out = os.path.join(WORK, "dump.txt")
        driver("dump", gz, contig, out)
        with open(out, "rb") as handle:
            arrays[f"dump_{key}_{contig}"] = np.frombuffer(handle.read(), dtype=np.uint8)
        meta["dump"].append({"file": key, "contig": contig})
    return gz


def make_allowlist(key, raw):
    path = os.path.join(WORK, key + ".txt")
    with open(path, "wb") as handle:
        handle.write(raw)
    arrays[f"allow_{key}"] = np.frombuffer(raw, dtype=np.uint8)
    meta["allowlists"][key] = {"entries": len(fx.parse_allowlist(raw))}
    return path


# "mixed": five contigs, one absent from the sizes file, one with a single line; every trap on chrA; weights that reach 2^24
big = [(150000, b"chrA\t150000\t150300\t" + BARCODES[3] + b"\t16777216"), (150100, b"chrA\t150100\t150400\t" + BARCODES[3] + b"\t16777217")]
mixed_text = text_of([("chrA", plain_lines("chrA", 1500, 100, 140000) + odd_lines("chrA", 1000, 139000) + big),
                      ("chrB", plain_lines("chrB", 400, 0, 59000) + plain_lines("chrB", 40, 0, 59000, fields=3)),
                      ("chrC", [(777, b"chrC\t777\t999\t" + BARCODES[0] + b"\t2")]),
                      ("chrD", plain_lines("chrD", 300, 50, 20000)),
                      ("chrE", plain_lines("chrE", 200, 10, 29000, fields=4))], terminated=False)
MIXED = make_file("mixed", mixed_text)

# "blocks": the same kind of text re-blocked: a line and a digit run straddle blocks, chrB begins mid-block, chrC on a block's
# first byte, small blocks besides
blocks_text = text_of([("chrA", plain_lines("chrA", 600, 100, 90000) + odd_lines("chrA", 500, 80000)),
                       ("chrB", plain_lines("chrB", 300, 0, 59000)), ("chrC", plain_lines("chrC", 200, 0, 40000))], inner_meta=True)
first_c = blocks_text.index(b"\nchrC\t") + 1
first_b = blocks_text.index(b"\nchrB\t") + 1
digit_run = blocks_text.index(b"\t", blocks_text.index(b"\nchrA\t") + 6) + 3  # inside the second column of the second chrA line
cuts = sorted({digit_run, 4096, 4097, 9000, first_b - 700, first_b + 800, first_c} | set(range(12000, first_b - 1000, 5000)))
assert all(0 < c < len(blocks_text) for c in cuts) and blocks_text[digit_run - 1: digit_run + 1].isdigit()
BLOCKS = make_file("blocks", blocks_text, cuts)

# "plain": what a pipeline writes: five fields, no header
plain_text = text_of([("chrA", plain_lines("chrA", 3000, 0, 190000)), ("chrE", plain_lines("chrE", 500, 0, 29000))], header=(), inner_meta=False)
PLAIN = make_file("plain", plain_text)
# "novalid": a contig whose every line is skipped (end == start): a range of 0 / 0 for a contig the index knows
novalid_text = text_of([("chrA", plain_lines("chrA", 60, 0, 5000)),
                        ("chrB", [(s, b"chrB\t%d\t%d\t" % (s, s) + BARCODES[0] + b"\t1") for s in range(100, 2100, 100)])], header=(), inner_meta=False)
NOVALID = make_file("novalid", novalid_text)
FILES = {"mixed": MIXED, "blocks": BLOCKS, "plain": PLAIN, "novalid": NOVALID}
TEXTS = {"mixed": mixed_text, "blocks": blocks_text, "plain": plain_text, "novalid": novalid_text}

# "unindexed": for the read-length probe alone (needs no index): end < start, end == start, short lines, a header
unindexed_text = (b"# header\nchrA\t50\t40\tx\t1\nchrA\t60\t60\nchrA\t70\nchrA\t\t90\n" +
                  b"".join(b"chrA\t%d\t%d\n" % (100 + 7 * i, 100 + 7 * i + 30 + (i * 37) % 211) for i in range(45)))
with open(os.path.join(WORK, "unindexed.tsv"), "wb") as handle:
    handle.write(unindexed_text)
driver("compress", os.path.join(WORK, "unindexed.tsv"), os.path.join(WORK, "unindexed.tsv.gz"))
arrays["file_unindexed_gz"] = np.fromfile(os.path.join(WORK, "unindexed.tsv.gz"), dtype=np.uint8)
FILES["unindexed"], TEXTS["unindexed"] = os.path.join(WORK, "unindexed.tsv.gz"), unindexed_text

ALLOW = {
    "empty": make_allowlist("empty", b"# nothing but comments\n\n   \n"),
    "one": make_allowlist("one", BARCODES[3] + b"\n"),
    "absent": make_allowlist("absent", b"NO-SUCH-BARCODE-1\n"),
    "many": make_allowlist("many", b"# cluster 7\n" + b"".join(b + b"\n" for i, b in enumerate(BARCODES) if i % 4 != 3) + b"  " + BARCODES[5] + b" trailing words\n" +
                           b"\t" + BARCODES[7] + b"\r\n" + BARCODES[8] + b"\n" + BARCODES[7][:4] + b"\n" + BARCODES[9] + b"\n" + BARCODES[9] + b"\n" +
                           LONG_BARCODE[:3000] + b"\n#" + BARCODES[11] + b"\n" + BARCODES[13]),
}
ALLOW_SETS = {key: fx.parse_allowlist(bytes(arrays[f"allow_{key}"])) for key in ALLOW}
ALLOW_SETS["-"] = set()
assert BARCODES[7][:4] in ALLOW_SETS["many"] and BARCODES[7] in ALLOW_SETS["many"]  # an entry that is a proper prefix of another

census = {}
MODE_NAMES = ["coverage", "cutsite", "fiveprime", "center"]


def contig_lines(key, contig):
    return [line for line in fx.split_lines(TEXTS[key]) if line.startswith(b"#") or line.split(b"\t")[0] == contig.encode()]


def count_scenario(name, key, contig, start, end, step, mode, one, allow="-", length=None):
    length = ((end - start - 1) // step) + 1 if length is None else length
    out = os.path.join(WORK, "counts.f32")
    said = driver("count", FILES[key], ALLOW.get(allow, "-"), contig, start, end, step, length, out, mode, one)
    record = {"name": name, "file": key, "contig": contig, "start": start, "end": end, "step": step, "mode": MODE_NAMES[mode],
              "one_read_per_bin": one, "allow": allow, "length": length}
    if said.startswith("ERROR"):
        record["error"] = said[6:]
    else:
        counts = np.fromfile(out, dtype=np.float32)
        arrays[f"c_{name}"] = counts
        mine = fx.count_region(contig_lines(key, contig), ALLOW_SETS[allow], start, end, step, length, mode, one, census)
        assert np.array_equal(mine, counts), f"tests/fragments_expected.py and the reference disagree on {name}"
    meta["count"].append(record)


n = 0
for mode in range(4):
    for one in (0, 1):
        for allow in ("-", "many"):
            count_scenario(f"blocks_chrA_{n}", "blocks", "chrA", 0, 100000, 50, mode, one, allow)
            count_scenario(f"mixed_chrA_{n}", "mixed", "chrA", 1237, 61761, 10, mode, one, allow)           # off 0, cuts fragments at both edges
            n += 1
for mode in range(4):
    count_scenario(f"mixed_edge_{mode}", "mixed", "chrA", 20000, 30000, 1000, mode, 0, "one")                # ends on a bin edge
    count_scenario(f"mixed_clamp_{mode}", "mixed", "chrA", 0, 140000, 50, mode, 0, "-", length=1217)          # countBufferLength clamps index1
    count_scenario(f"mixed_clamp_one_{mode}", "mixed", "chrA", 0, 140000, 50, mode, 1, "empty", length=1217)
    count_scenario(f"mixed_step1_{mode}", "mixed", "chrA", 58000, 61000, 1, mode, 0, "many")
    count_scenario(f"mixed_big_{mode}", "mixed", "chrA", 149000, 151000, 50, mode, 0)                         # weights 2^24 and 2^24 + 1
    count_scenario(f"mixed_chrC_{mode}", "mixed", "chrC", 0, 50000, 50, mode, 0)
    count_scenario(f"mixed_chrD_{mode}", "mixed", "chrD", 0, 25000, 10, mode, 0, "many")
    count_scenario(f"mixed_chrE_{mode}", "mixed", "chrE", 33, 29777, 50, mode, 0, "many")
    count_scenario(f"blocks_chrB_{mode}", "blocks", "chrB", 0, 60000, 50, mode, 0)                            # begins mid-block
    count_scenario(f"blocks_chrC_{mode}", "blocks", "chrC", 0, 50000, 1000, mode, 1)                          # begins on a block's first byte
    count_scenario(f"plain_chrA_{mode}", "plain", "chrA", 0, 200000, 50, mode, 0)
    count_scenario(f"plain_empty_region_{mode}", "plain", "chrE", 29900, 30000, 10, mode, 0)
count_scenario("unknown_contig", "mixed", "chrNone", 0, 1000, 50, 0, 0)


def range_scenario(key, contig, chrom_len, allow="-"):
    said = driver("range", FILES[key], ALLOW.get(allow, "-"), contig, chrom_len)
    a, b = (int(v) for v in said.split())
    kept = [line for line in contig_lines(key, contig) if line.startswith(b"#") or int(line.split(b"\t")[1]) < chrom_len]
    assert fx.chrom_range(kept, census) == (a, b), (key, contig, chrom_len, fx.chrom_range(kept), (a, b))
    meta["range"].append({"file": key, "contig": contig, "chrom_len": chrom_len, "allow": allow, "start": a, "end": b})


for key, contig, chrom_len in [("mixed", "chrA", 200000), ("mixed", "chrA", 100000), ("mixed", "chrA", 1500), ("mixed", "chrB", 60000),
                               ("mixed", "chrC", 50000), ("mixed", "chrC", 700), ("mixed", "chrD", 999999), ("mixed", "chrE", 30000),
                               ("mixed", "chrNone", 1000), ("blocks", "chrA", 200000), ("blocks", "chrB", 60000), ("blocks", "chrC", 50000),
                               ("plain", "chrA", 200000), ("plain", "chrE", 30000), ("novalid", "chrB", 60000), ("novalid", "chrA", 200000)]:
    range_scenario(key, contig, chrom_len)
range_scenario("mixed", "chrA", 200000, "many")

# the [count_start, count_end) windows get_bam_chrom_reads derives from the ranges (rocco/readtracks.py:467-473)
for r in list(meta["range"]):
    if r["end"] > r["start"] and r["contig"] in SIZES and r["allow"] == "-" and r["chrom_len"] == SIZES[r["contig"]]:
        for step in (1, 10, 50, 1000):
            count_start = max(0, (r["start"] // step) * step)
            count_end = min(SIZES[r["contig"]], int(np.ceil(max(r["end"], count_start + 1) / float(step)) * step))
            if step == 1 and count_end - count_start > 70000:
                continue
            count_scenario(f"window_{r['file']}_{r['contig']}_{step}", r["file"], r["contig"], count_start, count_end, step, 0, 0)


def mapped_scenario(key, mode, one, allow="-", exclude=()):
    said = driver("mapped", FILES[key], ALLOW.get(allow, "-"), mode, one, *exclude)
    record = {"file": key, "mode": MODE_NAMES[mode], "one_read_per_bin": one, "allow": allow, "exclude": list(exclude)}
    if said.startswith("ERROR"):
        record["error"] = said[6:]
    else:
        record["mapped"], record["unmapped"] = (int(v) for v in said.split())
        mine = fx.mapped_count(fx.split_lines(TEXTS[key]), ALLOW_SETS[allow], {e.encode() for e in exclude}, mode, one, census)
        assert mine == record["mapped"], (record, mine)
    meta["mapped"].append(record)


for key in ("mixed", "blocks", "plain"):
    for mode in range(4):
        for one in (0, 1):
            mapped_scenario(key, mode, one)
            mapped_scenario(key, mode, one, "many", ("chrB", "chrX"))
    mapped_scenario(key, 0, 0, "one", ("chrA",))
    mapped_scenario(key, 0, 0, "empty", ("chr",))
mapped_scenario("unindexed", 0, 0)


def readlen_scenario(key, min_reads, max_iterations):
    said = driver("readlen", FILES[key], min_reads, max_iterations)
    record = {"file": key, "min_reads": min_reads, "max_iterations": max_iterations}
    if said.startswith("ERROR"):
        record["error"] = said[6:]
    else:
        record["read_length"] = int(said)
        assert fx.read_length(fx.split_lines(TEXTS[key]), min_reads, max_iterations, census) == record["read_length"], record
    meta["readlen"].append(record)


for key in ("mixed", "blocks", "plain", "unindexed"):
    for min_reads, max_iterations in ((32, 4096), (33, 4096), (1, 1), (2, 1), (0, 0), (5000, 10000), (40, 7)):
        readlen_scenario(key, min_reads, max_iterations)
header_only = os.path.join(WORK, "header_only.tsv")
with open(header_only, "wb") as handle:
    handle.write(b"# nothing else\nchrA\t5\n")
driver("compress", header_only, header_only + ".gz")
arrays["file_header_only_gz"] = np.fromfile(header_only + ".gz", dtype=np.uint8)
FILES["header_only"], TEXTS["header_only"] = header_only + ".gz", b"# nothing else\nchrA\t5\n"
readlen_scenario("header_only", 32, 4096)

# ---- 3. the Python level: the reference's own readtracks.py over a stand-in native module --------------------------------
# (the method of make_golden_alignment_counts.py step 3: `_require_native_counter` is replaced IN THE MODULE by a stand-in that
# forwards every call to the driver with the fragments source kind, the scenario's allow-list and the scenario's count mode)
import importlib  # noqa: E402
import logging  # noqa: E402
import types  # noqa: E402

pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco")]
sys.modules["rocco"] = pkg
rt = importlib.import_module("rocco.readtracks")
SIZES_FILE = os.path.join(WORK, "t.sizes")
with open(SIZES_FILE, "w") as handle:
    for name, length in SIZES.items():
        handle.write(f"{name}\t{length}\n")
    handle.write("chrX\t1000\n")


def refused(said):
    if said.startswith("ERROR"):
        raise RuntimeError(said[6:])
    return said


class Native:
    """The compiled counter's answers for a fragments source (the driver), under one allow-list and one count mode."""

    def __init__(self, allow, mode):
        self.allow, self.mode = ALLOW.get(allow, "-"), mode

    def is_alignment_paired_end(self, *_a, **_k):
        return False  # (ccounts_isPairedEnd answers 0 for a source that is no alignment file: ccounts_backend.c:614-617)

    def get_alignment_read_length(self, path, min_reads=32, thread_count=1, max_iterations=4096, flag_exclude=0):
        return int(refused(driver("readlen", path, min_reads, max_iterations)))

    def get_alignment_mapped_read_count(self, path, exclude_chromosomes=(), thread_count=1, count_mode="coverage", one_read_per_bin=0):
        mapped, unmapped = refused(driver("mapped", path, self.allow, MODE_NAMES.index(count_mode), one_read_per_bin, *exclude_chromosomes)).split()
        return int(mapped), int(unmapped)

    def get_alignment_fragment_length(self, *_a, **_k):
        raise RuntimeError("source kind is not BAM")  # (ccounts_getFragmentLength: ccounts_backend.c:968-971)

    def get_alignment_chrom_range(self, path, chromosome, chrom_size, thread_count=1, flag_exclude=0):
        a, b = refused(driver("range", path, self.allow, chromosome, chrom_size)).split()
        return int(a), int(b)

    def count_alignment_region(self, path, chromosome, start, end, step, read_length, one_read_per_bin=0, thread_count=1, count_mode="coverage", **_k):
        out = os.path.join(WORK, "tail.f32")
        length = ((end - start - 1) // step) + 1
        refused(driver("count", path, self.allow, chromosome, start, end, step, length, out, self.mode, one_read_per_bin))
        return np.fromfile(out, dtype=np.float32)


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.INFO)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


meta["tail"] = []
rt.logger.setLevel(logging.INFO)


def tail_scenario(name, key, contig, step, mode=0, allow="-", **kwargs):
    rt._BAM_COUNT_METADATA_CACHE.clear()
    native = Native(allow, mode)
    rt._require_native_counter = lambda: native
    keep = Keep()
    rt.logger.addHandler(keep)
    path = FILES[key]
    call = dict(effective_genome_size=2.7e9, norm_method="RPGC", min_mapping_score=10, flag_include=None, flag_exclude=3844, extend_reads=-1,
                center_reads=False, ignore_for_norm=None, scale_factor=1.0, num_processors=1, const_scale=1.0, round_digits=5, scale_by_step=False)
    call.update(kwargs)
    record = {"name": name, "file": key, "contig": contig, "step": step, "mode": MODE_NAMES[mode], "allow": allow, "kwargs": kwargs}
    try:
        intervals, vals = rt.get_bam_chrom_reads(path, contig, SIZES_FILE, step, **call)
        metadata = rt._get_bam_count_metadata(path, step=step, norm_method=call["norm_method"], effective_genome_size=call["effective_genome_size"],
                                              ignore_for_norm=call["ignore_for_norm"] or ["chrX", "chrY", "chrM"], flag_exclude=call["flag_exclude"],
                                              extend_reads=call["extend_reads"], num_processors=1, scale_factor=call["scale_factor"])
        record["metadata"] = {k: metadata[k] for k in ("paired_end", "paired_end_mode", "read_length", "norm_read_length", "resolved_extend_bp",
                                                       "mapped_reads", "norm_scale", "threads")}
        if intervals is None:
            record["none"] = True
        else:
            arrays[f"t_{name}_intervals"], arrays[f"t_{name}_values"] = np.asarray(intervals), np.asarray(vals)
            record["intervals_dtype"], record["values_dtype"] = str(np.asarray(intervals).dtype), str(np.asarray(vals).dtype)
    except Exception as exc:  # noqa: BLE001  (the type and the words are what is stored)
        record["exception"] = [type(exc).__name__, str(exc).replace(path, "{file}").replace(SIZES_FILE, "{sizes}")]
    rt.logger.removeHandler(keep)
    record["log"] = [[level, message.replace(path, "{file}")] for level, message in keep.records]
    meta["tail"].append(record)


tail_scenario("plain_coverage", "plain", "chrA", 50)
tail_scenario("plain_cutsite_list", "plain", "chrA", 10, 1, "many", norm_method="CPM")
tail_scenario("plain_fiveprime", "plain", "chrE", 1, 2, norm_method="RPKM")
tail_scenario("plain_center_mode", "plain", "chrA", 1000, 3, "many", norm_method="BPM")
tail_scenario("plain_center_reads", "plain", "chrA", 50, 0, center_reads=True, norm_method="CPM")
tail_scenario("plain_center_reads_cutsite", "plain", "chrE", 50, 1, "one", center_reads=True, norm_method="CPM")
tail_scenario("blocks_coverage_list", "blocks", "chrA", 50, 0, "many", norm_method="RPKM", ignore_for_norm=["chrB"])
tail_scenario("blocks_mid_block_contig", "blocks", "chrB", 10, 1, norm_method="CPM", scale_by_step=True)
tail_scenario("blocks_block_start_contig", "blocks", "chrC", 50, 3, norm_method="CPM", const_scale=0.0)
tail_scenario("mixed_list", "mixed", "chrA", 50, 0, "many", norm_method="CPM", scale_factor=2.5, round_digits=2)
tail_scenario("mixed_single_line", "mixed", "chrC", 50, 1, "many", norm_method="CPM", const_scale=-2.0)
tail_scenario("mixed_four_fields", "mixed", "chrE", 1000, 2, "many", extend_reads=150)
tail_scenario("unknown_contig", "plain", "chrB", 50, norm_method="CPM")                        # (None, None): the index does not know it
tail_scenario("no_valid_line", "novalid", "chrB", 50, norm_method="CPM")                       # (None, None): a range of 0 / 0
tail_scenario("no_positive_value", "plain", "chrE", 50, 0, "absent", norm_method="CPM")        # (None, None): nothing passes the list
tail_scenario("extend_reads_zero", "plain", "chrA", 50, extend_reads=0)                        # RuntimeError: source kind is not BAM
tail_scenario("rpgc_without_genome_size", "plain", "chrA", 50, effective_genome_size=-1)       # ValueError
tail_scenario("contig_not_in_sizes", "mixed", "chrD", 50, 0, "many", norm_method="CPM")        # ValueError
tail_scenario("no_index", "unindexed", "chrA", 50, norm_method="CPM")                          # RuntimeError: no tabix index

# ---- 4. the census -----------------------------------------------------------------------------------------------------
NEEDED = ["count:meta", "count:last_empty", "count:end_le_start", "count:barcode", "center:in", "center:outside", "cut:start:in",
          "cut:start:outside", "cut:end:in", "cut:end:outside", "coverage:in", "coverage:outside", "coverage:clipped",
          "coverage:index0_beyond", "coverage:index1_clamped", "center:beyond_buffer", "mapped:excluded", "mapped:short",
          "mapped:fifth_empty", "mapped:barcode", "mapped:in",
          # the range consumer reads index spans only: a line without three parsable fields cannot be indexed, so its rules
          # are the meta line and end <= start; the read-length consumer reads any file
          "range:meta", "range:end_le_start", "range:in", "readlen:start", "readlen:end", "readlen:end_le_start", "readlen:in"]
missing = [rule for rule in NEEDED if census.get(rule, 0) == 0]
assert not missing, f"the fixture files never meet: {missing}"
meta["census"] = {rule: int(census[rule]) for rule in sorted(census)}

np.savez_compressed(os.path.join(HERE, "fragments.npz"), **arrays)
with open(os.path.join(HERE, "fragments.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(meta['count'])} count, {len(meta['range'])} range, {len(meta['mapped'])} mapped and {len(meta['readlen'])} readlen scenarios, "
      f"{len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'fragments.npz'))} bytes")
print("census", meta["census"])
print("errors", [(r.get("name", r.get("file")), r["error"]) for kind in ("count", "mapped", "readlen") for r in meta[kind] if "error" in r])
