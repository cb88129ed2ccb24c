#!/usr/bin/env python3
"""What the REFERENCE's ``ccounts_getCellCount`` makes of fragments files (note (35)).

    python tests/golden/make_golden_barcode_census.py        (by hand, where the reference is mounted; under a minute)

Every stored result was written by the reference's compiled C:

1. The reference's vendored htslib is copied into a temporary directory and built as make_golden_fragments.py builds it; the
   reference's ``native/ccounts_backend.c`` is compiled against it together with this project's driver
   (tests/golden/barcode_census_driver.c).  Nothing built or copied there is kept.
2. Small seeded texts become BGZF files with a ``.tbi`` (the driver's ``pack``); the driver calls ``ccounts_getCellCount``
   (``cells``) for every file under every allow-list, for a file without an index and for a BAM file (the errors are stored
   as the reference words them), and, for the file whose every fifth column is 1, ``ccounts_getMappedReadCount`` under each
   one-barcode allow-list: the reference's own count of records per barcode.
3. tests/barcode_census_expected.py replays every call; a disagreement stops this script.

htslib indexes a line only if its first three columns parse, so every trap stands in column 4 or behind it, or on a ``#``
line (which the index skips and ``hts_getline`` reads).

Writes tests/golden/barcode_census.npz + .json (data only: the bytes of every .tsv.gz, .tbi and allow-list, and every result)."""
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
import barcode_census_expected as bx  # noqa: E402
import fragments_expected as fx  # noqa: E402

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="barcode_census_")

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
                os.path.join(HERE, "barcode_census_driver.c"), os.path.join(REFERENCE, "rocco", "native", "ccounts_backend.c"),
                os.path.join(HTS, "libhts.a"), "-lz", "-lm", "-lpthread", "-o", DRIVER], check=True)


def driver(*args):
    return subprocess.run([DRIVER, *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout.strip()


# ---- 2. the texts ------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(20262)
LONG_A = bytes(rng.choice(list(b"ACGT"), size=299).astype(np.uint8)) + b"A"   # 300 bytes, equal to LONG_C but for the last
LONG_C = LONG_A[:-1] + b"C"
TRAPS = [b"G", b"AC", b"ACG", b"ACGT", LONG_A, LONG_C, b"\xc3\xa9\xffB", b"\x80", b"TTTTTTTTTTTTTTTA-1", b"TTTTTTTTTTTTTTTC-1", b"A B", b"#hash", b"-"]
PLAIN = [("".join(rng.choice(list("ACGT"), size=16)) + "-1").encode() for _ in range(40)]
arrays, meta = {}, {"files": {}, "allowlists": {}, "cells": [], "per_barcode": []}


def body_lines(contig, barcodes, n, lo, hi, fifth=None):
    out = []
    for s in np.sort(rng.integers(lo, hi, size=n)):
        barcode = barcodes[int(rng.integers(0, len(barcodes)))]
        out.append((int(s), b"%s\t%d\t%d\t%s\t%d" % (contig, s, s + int(rng.integers(20, 600)), barcode, fifth or int(rng.integers(1, 6)))))
    return out


def trap_lines(contig, lo, hi):
    """What the issue lists, each a few times at seeded places: every tail stands behind three sound columns."""
    out = []
    tails = [b"", b"\t", b"\t\t4", b"\t\t", b"\tACG", b"\tG", b"\tAC\r", b"\tACGT\t1\r", b"\r", b"\tAC\rGT\t1", b"\t\rAC\t1", b"\tG\t1\r2",
             b"\tACG\x00T\t1", b"\t\x00ACGT\t1", b"\tAC\t1\x00", b"\x00\tACGT\t1", b"\tA B\t1", b"\t#hash\t2", b"\t-", b"\tACGT\tx\ty\tz"]
    tails += [b"\t" + t + b"\t1" for t in TRAPS] + [b"\t" + t for t in TRAPS]
    for tail in tails:
        for _ in range(2):
            s = int(rng.integers(lo, hi))
            out.append((s, b"%s\t%d\t%d" % (contig, s, s + 50) + tail))
    return out


def text_of(per_contig, header, terminated=True):
    lines = list(header)
    for contig, entries in per_contig:
        body = [e[1] for e in sorted(entries, key=lambda e: e[0])]
        body.insert(len(body) // 2, b"#" + contig + b"\t0\t0\tMETA-INSIDE\t1")
        lines += body
    text = b"".join(line + b"\n" for line in lines)
    return text if terminated else text[:-1]


HEADER = (b"# a header line", b"#chrA\t1\t2\tMETA-FOUR-FIELDS", b"#\t\t\tACG\t7", b"#three\tfields\tonly")
TEXTS, FILES = {}, {}


def make_file(key, text, cuts=(), index=True):
    txt, gz = os.path.join(WORK, key + ".tsv"), os.path.join(WORK, key + ".tsv.gz")
    with open(txt, "wb") as handle:
        handle.write(text)
    driver("pack" if index else "compress", txt, gz, *cuts)
    arrays[f"file_{key}_gz"] = np.fromfile(gz, dtype=np.uint8)
    if index:
        arrays[f"file_{key}_tbi"] = np.fromfile(gz + ".tbi", dtype=np.uint8)
    meta["files"][key] = {"cuts": [int(c) for c in cuts], "indexed": bool(index), "bytes": len(text), "lines": bx.lines_of(text)}
    TEXTS[key], FILES[key] = text, gz


# "traps": every trap, an unterminated last line, one small block and htslib's own behind it.  The traps stand on the second
# contig: htslib takes a file whose leading bytes hold a NUL for a binary one and the reference then fails to open it
make_file("traps", text_of([(b"chrA", body_lines(b"chrA", PLAIN[4:12] + TRAPS[:4], 70, 0, 50000)),
                            (b"chrB", body_lines(b"chrB", PLAIN[:8], 60, 100, 90000) + trap_lines(b"chrB", 500, 80000))], HEADER, terminated=False),
          [2500])
assert b"\x00" not in TEXTS["traps"][:2500]
# "blocks": the same kind of text in blocks of about 2 500 bytes, cut wherever that falls: lines straddle blocks, and the
# barcodes of the first block return in every later one
blocks_text = text_of([(b"chrA", body_lines(b"chrA", PLAIN[:12] + TRAPS[:6], 220, 100, 90000) + trap_lines(b"chrA", 500, 80000)),
                       (b"chrB", body_lines(b"chrB", PLAIN[:12] + TRAPS[4:10], 150, 0, 50000)),
                       (b"chrC", body_lines(b"chrC", PLAIN, 150, 0, 40000))], HEADER)
make_file("blocks", blocks_text, list(range(2500, len(blocks_text), 2500)))
# "ones": what a pipeline writes, every fifth column 1, a dozen barcodes: the mapped count under a one-barcode list is the
# reference's own number of records of that barcode
ONES = PLAIN[20:32]
make_file("ones", text_of([(b"chrA", body_lines(b"chrA", ONES, 300, 0, 90000, fifth=1)), (b"chrB", body_lines(b"chrB", ONES[:5], 80, 0, 9000, fifth=1))],
                          header=()).replace(b"#chrA\t0\t0\tMETA-INSIDE\t1\n", b"").replace(b"#chrB\t0\t0\tMETA-INSIDE\t1\n", b""))
# "nobarcode": three-field lines and empty barcodes only
make_file("nobarcode", b"# nothing to count\n" + b"".join(b"chrA\t%d\t%d%s\n" % (10 * i, 10 * i + 5, (b"", b"\t", b"\t\t3")[i % 3]) for i in range(30)))
make_file("unindexed", TEXTS["ones"], index=False)


def make_allowlist(key, raw):
    path = os.path.join(WORK, "allow_" + key + ".txt")
    with open(path, "wb") as handle:
        handle.write(raw)
    arrays[f"allow_{key}"] = np.frombuffer(raw, dtype=np.uint8)
    meta["allowlists"][key] = {"entries": len(fx.parse_allowlist(raw))}
    return path


ALLOW = {
    "empty": make_allowlist("empty", b""),
    "nothing": make_allowlist("nothing", b"NO-SUCH-BARCODE-1\nACGTT\n"),
    "prefix": make_allowlist("prefix", b"ACG\nTTTTTTTTTTTTTTT\n" + LONG_A[:200] + b"\n"),
    "some": make_allowlist("some", b"# a cluster\n" + b"".join(b + b"\n" for b in PLAIN[::3]) + b"G\nAC\n" + LONG_C + b"\n\xc3\xa9\xffB\n\x80\n  TTTTTTTTTTTTTTTA-1 x\n-\n"),
}
ALLOW_SETS = {key: fx.parse_allowlist(bytes(arrays[f"allow_{key}"])) for key in ALLOW}
ALLOW_SETS["-"] = set()

# ---- 3. the reference's answers, each replayed by the statement ---------------------------------------------------------
for key in ("traps", "blocks", "ones", "nobarcode", "unindexed"):
    for allow in ("-", "empty", "nothing", "prefix", "some"):
        said = driver("cells", FILES[key], ALLOW.get(allow, "-"), "fragments")
        record = {"file": key, "allow": allow}
        if said.startswith("ERROR"):
            record["error"] = said[6:].replace(FILES[key], "{file}")
        else:
            record["cells"] = int(said)
            mine = bx.census(TEXTS[key], ALLOW_SETS[allow])
            assert len(mine) == record["cells"], f"tests/barcode_census_expected.py and the reference disagree on {record}: {len(mine)}"
        meta["cells"].append(record)
bam = os.path.join(WORK, "some.bam")
np.load(os.path.join(HERE, "bam_files.npz"))["bam_mixed"].tofile(bam)
meta["cells"].append({"file": "bam", "allow": "-", "error": driver("cells", bam, "-", "bam")[6:].replace(bam, "{file}")})

mine = bx.census(TEXTS["ones"])
assert 2 <= len(mine) <= 12
for barcode in sorted(mine):
    path = os.path.join(WORK, "single.txt")
    with open(path, "wb") as handle:
        handle.write(barcode + b"\n")
    mapped, unmapped = (int(v) for v in driver("mapped", FILES["ones"], path).split())
    assert mapped == mine[barcode] and unmapped == 0, (barcode, mapped, mine[barcode])
    meta["per_barcode"].append({"file": "ones", "barcode": barcode.decode("ascii"), "records": mapped})

# what the texts must contain (the issue's list), by the statement
traps = bx.census(TEXTS["traps"])
for needed in TRAPS + [b"META-FOUR-FIELDS", b"META-INSIDE"]:
    assert needed in traps, needed
assert b"ACGT" in traps and b"GT" not in traps and b"T" not in traps and not TEXTS["traps"].endswith(b"\n")
assert b"\x00" in TEXTS["traps"] and b"\r\n" in TEXTS["traps"] and b"AC\rGT" in TEXTS["traps"] and any(len(b) == 300 for b in traps)
assert bx.census(TEXTS["nobarcode"]) == {}

np.savez_compressed(os.path.join(HERE, "barcode_census.npz"), **arrays)
with open(os.path.join(HERE, "barcode_census.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(meta['cells'])} cell counts and {len(meta['per_barcode'])} per-barcode counts, {len(arrays)} arrays, "
      f"{os.path.getsize(os.path.join(HERE, 'barcode_census.npz'))} bytes")
print("cells", [(r["file"], r["allow"], r.get("cells", r.get("error"))) for r in meta["cells"]])
