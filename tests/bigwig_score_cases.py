"""(not a test module) The bigWig files and calls behind tests/golden/bigwig_scores.npz / .json (note (31)):
tests/golden/make_golden_bigwig_scores.py writes these files with the writer of bigwig_files.py, reads them with its second reader and
hands the intervals to the REFERENCE's `get_bigwig_chrom_scores` / `generate_chrom_matrix` through a stand-in pyBigWig; the tests write
the same files again (checked by `digest`) and hold rocco_amd.bigwig's functions of the same names against what the reference returned.
Every value is a float32, every file's starts ascend except where the case is the error itself."""
import hashlib
import os

import numpy as np

import bigwig_files as bf

BIG = 10 ** 7
SIZES = [("chr1", BIG), ("chrA", 9000), ("chrB", 9000), ("chrE", 1000), ("c0", 50000), ("c1", 50000), ("c2", 50000), ("chrNone", 12345)]
SIZES_FILE, OTHER_SIZES_FILE = "genome.sizes", "other.sizes"  # (the second lacks chrA)


def _fixed(n, first, step=50, span=None, seed=0, scale=10.0):
    rng = np.random.default_rng(seed)
    return bf.section(0, 3, bf.f32(rng.random(n) * scale), start=first, step=step, span=step if span is None else span)


def files():
    """{file name: (chroms, sections, keywords of `write_bigwig`)}; "notbigwig.bw" is text."""
    one = [("chr1", BIG)]
    mixed = bf.bed_sections(0, 2, 5, first=0, seed=1) + bf.var_sections(0, 2, 5, first=500, seed=2) + bf.fixed_sections(0, 2, 5, first=1000, seed=3)
    turns = [_fixed(63, 0, seed=11), _fixed(64, 63 * 50, seed=12), _fixed(65, 127 * 50, seed=13), _fixed(1024, 192 * 50, seed=14),
             dict(_fixed(6, 1216 * 50, seed=15), item_count=4)]  # (the last: two items' bytes behind what the header counts)
    edge = [bf.section(0, 2, [(800, np.float32(1.25)), (850, np.float32(2.5))], span=50),
            bf.section(0, 1, [(900, 950, 1.5), (950, 1000, 2.5), (1000, 1050, 3.5), (1050, 1100, 4.5)]),
            bf.section(0, 3, bf.f32([5, 6, 7]), start=1100, step=50, span=50, leaf=(0, 0, 0, 1000))]
    other = bf.fixed_sections(0, 1, 5, seed=6) + [bf.section(0, 3, bf.f32([1, 2, 3]), start=250, step=50, span=50, header_chrom=1)] + \
        bf.fixed_sections(0, 1, 5, first=400, seed=7)
    three = [("c0", 50000), ("c1", 50000), ("c2", 50000)]
    spread = [bf.section(0, 3, bf.f32([1, 2, 3, 4]), start=100, step=50, span=50), bf.section(2, 3, bf.f32([5, 6, 7]), start=200, step=50, span=50)]
    good = bf.f32([1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
    out = {
        "fixed.bw": (one, bf.fixed_sections(0, 3, 40, first=2000, seed=1), {}),
        "var.bw": (one, bf.var_sections(0, 3, 40, first=2000, seed=2), {}),
        "bed.bw": (one, bf.bed_sections(0, 3, 40, first=2000, seed=3), {}),
        "mixed.bw": (one, mixed, {}),
        "stored.bw": (one, mixed, dict(buf_size=0)),
        "gaps.bw": (one, bf.fixed_sections(0, 6, 9, seed=8, gap_every=2), {}),
        "turns.bw": (one, turns, {}),
        "edge.bigwig": ([("chrE", 1000)], edge, {}),
        "other.bw": ([("chrA", 9000), ("chrB", 9000)], other, {}),
        "three.bw": (three, spread, dict(key_size=8)),
        "nan.bw": (one, [bf.section(0, 3, bf.f32([1, np.nan, 2, 1, 0, 3]), start=0, step=25, span=25)], {}),
        "inf.bw": (one, [bf.section(0, 3, bf.f32([1, 2, np.inf, 1, 0, 3]), start=0, step=25, span=25)], {}),
        "span0.bw": (one, [bf.section(0, 3, good, start=0, step=25, span=0)], {}),
        "widths.bw": (one, [bf.section(0, 1, [(0, 25, 1.0), (25, 75, 2.0), (75, 100, 1.0)])], {}),
        "misaligned.bw": (one, [bf.section(0, 2, [(0, np.float32(1)), (30, np.float32(2)), (75, np.float32(1))], span=25)], {}),
        "duplicate.bw": (one, [bf.section(0, 2, [(0, np.float32(1)), (50, np.float32(2)), (50, np.float32(3))], span=25)], {}),
        "m_a.bw": (one, [_fixed(120, 1000, seed=21)], {}),
        "m_b.bw": (one, [_fixed(100, 1500, seed=22, scale=1000.0)], {}),
        "m_c.bigwig": (one, [_fixed(90, 800, seed=23, scale=0.01), _fixed(60, 800 + 90 * 50, seed=24)], {}),
        "m_step75.bw": (one, [_fixed(40, 0, step=75, seed=25)], {}),
        "m_empty.bw": ([("chr1", BIG), ("chr2", BIG)], [bf.section(1, 3, bf.f32([1, 2]), start=0, step=50, span=50)], {}),
        "m_lacks.bw": ([("chr2", BIG)], [bf.section(0, 3, bf.f32([1, 2]), start=0, step=50, span=50)], {}),
    }
    return out


def write_files(directory) -> dict:
    """Writes every file, the text file and the two sizes files into `directory`; returns {file name: path}."""
    paths = {}
    for name, (chroms, sections, how) in files().items():
        paths[name] = os.path.join(str(directory), name)
        bf.write_bigwig(paths[name], chroms, sections, **how)
    paths["notbigwig.bw"] = os.path.join(str(directory), "notbigwig.bw")
    with open(paths["notbigwig.bw"], "w", encoding="utf-8") as handle:
        handle.write("track type=wiggle_0\nfixedStep chrom=chr1 start=1 step=50\n1.0\n2.0\n")
    for name, rows in ((SIZES_FILE, SIZES), (OTHER_SIZES_FILE, [r for r in SIZES if r[0] != "chrA"])):
        paths[name] = os.path.join(str(directory), name)
        with open(paths[name], "w", encoding="utf-8") as handle:
            handle.write("".join(f"{chrom}\t{size}\n" for chrom, size in rows))
    return paths


def digest(path, chroms) -> str:
    """SHA-256 over the second reader's interval arrays of every chromosome of the file, in the file's order."""
    h = hashlib.sha256()
    for chrom, _ in chroms:
        for a in bf.as_arrays(bf.expected_intervals(path, chrom)):
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(b"|")
    return h.hexdigest()


def score_cases():
    """[(name, file name, chromosome, sizes file name, keywords)] for `get_bigwig_chrom_scores`; "missing.bw" and "missing.sizes" do
    not exist."""
    S = SIZES_FILE
    return [
        ("fixedStep alone", "fixed.bw", "chr1", S, {}),
        ("variableStep alone", "var.bw", "chr1", S, {}),
        ("bedGraph alone", "bed.bw", "chr1", S, {}),
        ("the three types mixed", "mixed.bw", "chr1", S, {}),
        ("a stored file", "stored.bw", "chr1", S, {}),
        ("gaps filled with zeros", "gaps.bw", "chr1", S, {}),
        ("sections of 63, 64, 65 and 1024 items, trailing bytes", "turns.bw", "chr1", S, {}),
        ("items at and beyond the chromosome's length", "edge.bigwig", "chrE", S, {}),
        ("a leaf whose section names another chromosome", "other.bw", "chrA", S, {}),
        ("the other chromosome of that file", "other.bw", "chrB", S, {}),
        ("a chromosome with no section", "three.bw", "c1", S, {}),
        ("a chromosome absent from the file", "three.bw", "chrNone", S, {}),
        ("a chromosome absent from the sizes file", "other.bw", "chrA", OTHER_SIZES_FILE, {}),
        ("const_scale 0.5", "gaps.bw", "chr1", S, dict(const_scale=0.5)),
        ("const_scale 1/3, round_digits 2", "fixed.bw", "chr1", S, dict(const_scale=1.0 / 3.0, round_digits=2)),
        ("const_scale 0", "var.bw", "chr1", S, dict(const_scale=0.0)),
        ("const_scale -1 is no scale", "bed.bw", "chr1", S, dict(const_scale=-1.0)),
        ("round_digits 0", "m_b.bw", "chr1", S, dict(round_digits=0)),
        ("round_digits 2", "mixed.bw", "chr1", S, dict(round_digits=2)),
        ("round_digits 5 on small values", "m_c.bigwig", "chr1", S, dict(round_digits=5)),
        ("a NaN", "nan.bw", "chr1", S, {}),
        ("an infinity", "inf.bw", "chr1", S, {}),
        ("an infinity scaled by 0", "inf.bw", "chr1", S, dict(const_scale=0.0)),
        ("a fixedStep span of 0", "span0.bw", "chr1", S, {}),
        ("variable widths", "widths.bw", "chr1", S, {}),
        ("a misaligned start", "misaligned.bw", "chr1", S, {}),
        ("an adjacent duplicate bin", "duplicate.bw", "chr1", S, {}),
        ("no bigWig file at the path", "missing.bw", "chr1", S, {}),
        ("no sizes file at the path", "fixed.bw", "chr1", "missing.sizes", {}),
        ("a file that is no bigWig file", "notbigwig.bw", "chr1", S, {}),
    ]


def matrix_cases():
    """[(name, file names, chromosome, keywords)] for `generate_chrom_matrix` (step 50, the sizes file SIZES_FILE)."""
    return [
        ("K = 1", ["m_a.bw"], "chr1", {}),
        ("K = 3 with ragged ends", ["m_a.bw", "m_b.bw", "m_c.bigwig"], "chr1", {}),
        ("one track without data", ["m_a.bw", "m_empty.bw", "m_b.bw"], "chr1", {}),
        ("one file lacks the chromosome", ["m_lacks.bw", "m_c.bigwig"], "chr1", dict(const_scale=0.5, round_digits=2)),
        ("none with data", ["m_empty.bw", "m_lacks.bw"], "chr1", {}),
        ("two binning schemes", ["m_a.bw", "m_step75.bw"], "chr1", {}),
        ("low_memory", ["m_a.bw", "m_b.bw", "m_c.bigwig"], "chr1", dict(low_memory=True)),
        ("mixed file types", ["m_a.bw", "reads.bam"], "chr1", {}),
        ("an unsupported file type", ["m_a.bw", "track.wig"], "chr1", {}),
        ("an error in the second file, a missing third", ["m_a.bw", "widths.bw", "missing.bw"], "chr1", {}),
        ("a missing second file behind a good first", ["m_a.bw", "missing.bw"], "chr1", {}),
    ]


def path_of(paths: dict, directory, name: str) -> str:
    return paths.get(name, os.path.join(str(directory), name))
