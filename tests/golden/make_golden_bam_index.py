#!/usr/bin/env python3
"""``.bai`` indexes written by htslib, and what htslib's index iterator yields through them.

    python tests/golden/make_golden_bam_index.py        (by hand, where the reference is mounted; about a minute)

1. The reference's vendored htslib is built in a temporary directory exactly as make_golden_bam_files.py builds it.  This
   project's bam_files_driver.c (SAM -> BAM, ``sam_index_build(path, 0)``) and bam_index_driver.c (the iterator dump, the
   index statistics) are linked against it.  Nothing built or copied there is kept.
2. For each of the eight files of bam_files.npz the driver's ``index`` command writes the ``.bai``.
3. Three new files written by htslib: five contigs, several BGZF blocks, a contig without reads between two with reads,
   placed-unmapped mates, an unplaced tail.  `wide` is htslib's own blocking; `shared` and `edges` are cut again with
   tests/bam_expected.py's bgzf_compress (as `blocks` of bam_files.npz is) so that contigs begin and end inside blocks,
   share a block, and one ends exactly on a block's end; htslib indexes and reads them back like any other.
4. Per file and reference: what ``sam_itr_queryi(idx, tid, 0, length)`` yields, as record ordinals in file order;
   ``hts_idx_get_stat``; ``hts_idx_get_n_no_coor``.
5. A census is asserted (and asserted again by tests/test_bam_index_host.py): among the fixture contigs at least one begins
   inside a block, one ends inside a block, two share one block, one has no bins.

Writes tests/golden/bam_index.npz + .json (data only: index bytes, the new files' BAM bytes, the dumps)."""
import ast
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bam_expected as bx  # noqa: E402
import bam_index_files as bif  # noqa: E402

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
WORK = tempfile.mkdtemp(prefix="bam_index_")

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
for binary, source in (("files", "bam_files_driver.c"), ("index", "bam_index_driver.c")):
    BINARIES[binary] = os.path.join(WORK, binary)
    subprocess.run(["cc", *SETTINGS["BASE_COMPILE_ARGS"], "-I", HTS, os.path.join(HERE, source), os.path.join(HTS, "libhts.a"), "-lz", "-lm",
                    "-lpthread", "-o", BINARIES[binary]], check=True)


def driver(*args, binary="files"):
    return subprocess.run([BINARIES[binary], *[str(a) for a in args]], check=True, capture_output=True, text=True).stdout


# ---- 3. the new files ----------------------------------------------------------------------------------------------------
rng = np.random.default_rng(20311)
CONTIGS = [("chrB", 120000), ("chrE", 30000), ("chrA", 400000), ("chrD", 50000), ("chrC", 90000)]  # (chrE, chrD: see below)
CIGARS = [("50M", 50), ("20M5D30M", 50), ("10S40M", 50), ("25M100N25M", 50), ("36M", 36), ("*", 50)]
BASES = np.array(list("ACGT"))


def reads(contig, length, count, prefix, seq_rate=0.25):
    """Both strands, pairs, placed-unmapped mates (flag 4 with a contig and a position), a few secondary records."""
    lines = []
    for i, pos0 in enumerate(np.sort(rng.integers(0, length - 600, size=count))):
        cigar, qlen = CIGARS[int(rng.integers(0, len(CIGARS)))]
        flag = 16 if rng.random() < 0.5 else 0
        rnext, pnext, tlen = "*", 0, 0
        if rng.random() < 0.5:
            flag |= 1 | 2 | (64 if rng.random() < 0.5 else 128)
            tlen = int(rng.integers(20, 900)) * (1 if rng.random() < 0.5 else -1)
            rnext, pnext = "=", int(max(1, pos0 + tlen))
        if rng.random() < 0.06:
            flag, cigar = (flag | 4 | 1) & ~2, "*"  # an unmapped mate, placed at its mate's position
        flag |= 256 if rng.random() < 0.03 else 0
        seq = "".join(BASES[rng.integers(0, 4, size=qlen)]) if rng.random() < seq_rate else "*"
        lines.append((int(pos0), f"{prefix}{i}\t{flag}\t{contig}\t{int(pos0) + 1}\t{int(rng.integers(0, 61))}\t{cigar}\t{rnext}\t{pnext}\t{tlen}\t{seq}\t*"))
    return lines


def unplaced(count):
    return [f"u{i}\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*" for i in range(count)]


BAMS, NEW = {}, []


def make_file(key, per_contig, tail=(), cuts_from=None):
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
        entry0 = bx.header(data)[2]
        offsets, _, _, _ = bx.walk(data, entry0)
        tid = bx.fields(data, offsets, len(CONTIGS))[0]["tid"]
        with open(bam, "wb") as handle:
            handle.write(bx.bgzf_compress(data, cuts_from(data, offsets, tid)))
    BAMS[key] = bam
    NEW.append(key)


def first_of(offsets, tid, t):
    return int(offsets[np.flatnonzero(tid == t)[0]])


# wide: htslib's own blocks (about 64 KiB of records each); chrE has no reads, between chrB and chrA
make_file("wide", {"chrB": reads("chrB", 120000, 900, "b", 0.5), "chrA": reads("chrA", 400000, 1500, "a", 0.5),
                   "chrD": reads("chrD", 50000, 40, "d"), "chrC": reads("chrC", 90000, 300, "c", 0.5)}, unplaced(25))
# shared: small blocks; chrD lies wholly inside the block that chrA ends in and chrC begins in
make_file("shared", {"chrB": reads("chrB", 120000, 120, "b"), "chrA": reads("chrA", 400000, 200, "a"), "chrD": reads("chrD", 50000, 6, "d"),
                     "chrC": reads("chrC", 90000, 80, "c")}, unplaced(7),
          cuts_from=lambda data, offsets, tid: [first_of(offsets, tid, 0) + 700, first_of(offsets, tid, 2) - 300, first_of(offsets, tid, 2) + 3000,
                                                first_of(offsets, tid, 3) - 500, first_of(offsets, tid, 4) + 900, len(data) - 100])
# edges: chrB ends exactly on a block's end (chrA begins a block), chrA ends on one too, the unplaced tail begins a block
make_file("edges", {"chrB": reads("chrB", 120000, 60, "b"), "chrA": reads("chrA", 400000, 90, "a"), "chrC": reads("chrC", 90000, 30, "c")},
          unplaced(3),
          cuts_from=lambda data, offsets, tid: [first_of(offsets, tid, 2), first_of(offsets, tid, 2) + 2000, first_of(offsets, tid, 4),
                                                int(offsets[np.flatnonzero(tid < 0)[0]])])

# ---- 2., 4. the indexes and the dumps -----------------------------------------------------------------------------------------
arrays, meta = {}, {"files": {}, "new_files": NEW}
OLD = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only", "cg", "decoy"]
for key in OLD:
    BAMS[key] = bx.write_bam(WORK, key)
census = {"begins_inside": [], "ends_inside": [], "share_a_block": [], "no_bins": []}
for key in OLD + NEW:
    bam = BAMS[key]
    driver("index", bam)
    with open(bam + ".bai", "rb") as handle:
        arrays[f"bai_{key}"] = np.frombuffer(handle.read(), dtype=np.uint8)
    with open(bam, "rb") as handle:
        raw = handle.read()
    if key in NEW:
        arrays[f"bam_{key}"] = np.frombuffer(raw, dtype=np.uint8)
    out = os.path.join(WORK, key + ".idx.txt")
    driver("dump", bam, out, binary="index")
    facts = bif.facts(raw)
    entry = {"refs": [], "contigs": [[n, l] for n, l in facts["contigs"]], "bgzf_blocks": len(facts["blocks"])}
    with open(out) as handle:
        for line in handle:
            words = line.split()
            if words[0] == "ref":
                t, has_stat, mapped, unmapped, n = (int(w) for w in words[1:6])
                ordinals = np.asarray(words[6:], dtype=np.int64)
                assert ordinals.size == n and t == len(entry["refs"])
                arrays[f"itr_{key}_{t}"] = ordinals
                entry["refs"].append({"has_stat": bool(has_stat), "mapped": mapped, "unmapped": unmapped, "records": n})
                # the iterator over a whole contig yields exactly the contig's records, in file order
                assert np.array_equal(ordinals, np.flatnonzero(facts["fields"]["tid"] == t)), (key, t)
            elif words[0] == "nocoor":
                entry["n_no_coor"] = int(words[1])
            else:
                entry["records"] = int(words[1])
    assert entry["n_no_coor"] == facts["n_no_coor"] and entry["records"] == len(facts["offsets"]), key
    meta["files"][key] = entry
    spans = facts["spans"]
    block_of = lambda v: v >> 16  # noqa: E731
    for t, span in enumerate(spans):
        name = f"{key}:{facts['contigs'][t][0]}"
        if span is None:
            census["no_bins"].append(name)
            continue
        if span[0] & 0xFFFF:
            census["begins_inside"].append(name)
        if span[1] & 0xFFFF:
            census["ends_inside"].append(name)
        later = [u for u in range(t + 1, len(spans)) if spans[u] is not None]
        if later and span[1] & 0xFFFF and block_of(span[1]) == block_of(spans[later[0]][0]):
            census["share_a_block"].append(name)
meta["census"] = census
assert all(census[k] for k in census), census
assert any(n.startswith(("wide", "shared", "edges")) for n in census["share_a_block"])
for key in NEW:
    assert meta["files"][key]["bgzf_blocks"] >= 4 and len(meta["files"][key]["contigs"]) >= 4, key
    assert meta["files"][key]["n_no_coor"] > 0 and meta["files"][key]["refs"][1]["records"] == 0, key
    assert sum(r["unmapped"] for r in meta["files"][key]["refs"]) > 0, key

np.savez_compressed(os.path.join(HERE, "bam_index.npz"), **arrays)
with open(os.path.join(HERE, "bam_index.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
shutil.rmtree(WORK)
print(f"wrote {len(OLD) + len(NEW)} indexes, {len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'bam_index.npz'))} bytes")
for k, v in census.items():
    print("  ", k, len(v), v[:6])
