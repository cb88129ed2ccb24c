"""What tests/test_gpu_bam_matrix.py and tests/test_bam_matrix_host.py share: the fixtures of
tests/golden/bam_matrix.npz (written by tests/golden/make_golden_bam_matrix.py from the reference's own
generate_chrom_matrix), seeded synthetic records whose supports are known by construction, the size at which the fill
kernel enters its second turn, and the NumPy statement of the host's merge of supports."""
import json
import os

import numpy as np

import bam_expected as bx
from launch_turns_cases import second_turn

HERE = os.path.dirname(os.path.abspath(__file__))
STEP = 50
_golden = None


def golden():
    """(arrays, meta) of tests/golden/bam_matrix.npz / .json, loaded once and left unchanged."""
    global _golden
    if _golden is None:
        arrays = np.load(os.path.join(HERE, "golden", "bam_matrix.npz"))
        with open(os.path.join(HERE, "golden", "bam_matrix.json"), encoding="utf-8") as handle:
            _golden = ({k: arrays[k] for k in arrays.files}, json.load(handle))
    return _golden


def write_files(root) -> dict:
    """Every BAM file the scenarios name (the old ones from bam_files.npz, the new ones from bam_matrix.npz) and the sizes
    file, written under ``root``: {key: path}."""
    arrays, meta = golden()
    out = {key: bx.write_bam(root, key) for key in meta["old_files"]}
    for key in meta["new_files"]:
        out[key] = os.path.join(str(root), key + ".bam")
        with open(out[key], "wb") as handle:
            handle.write(arrays[f"bam_{key}"].tobytes())
    out["sizes"] = os.path.join(str(root), "t.sizes")
    with open(out["sizes"], "w") as handle:
        handle.write("".join(f"{name}\t{length}\n" for name, length in meta["sizes"]))
    return out


# ---- the host merge ------------------------------------------------------------------------------------------------------
def union_of_supports(firsts, lasts) -> np.ndarray:
    """The reference's statement (rocco/readtracks.py:614) on grid indices."""
    return np.unique(np.concatenate([np.arange(a, b + 1, dtype=np.int64) for a, b in zip(firsts, lasts)]))


def columns_of_segments(seg_grid, seg_col, m) -> np.ndarray:
    """The grid index of every column of a segment table, one segment after the other."""
    ends = np.append(seg_col[1:], m)
    return np.concatenate([g + np.arange(e - c, dtype=np.int64) for g, c, e in zip(seg_grid, seg_col, ends)])


def seeded_supports(rng):
    """A support set with nested, identical, touching, overlapping and disjoint members."""
    k = int(rng.integers(1, 12))
    firsts = rng.integers(0, 400, size=k)
    lasts = firsts + rng.integers(0, 60, size=k)
    for i in range(1, k):
        kind = int(rng.integers(0, 6))
        j = int(rng.integers(0, i))
        if kind == 0:    # touching behind j
            firsts[i], lasts[i] = lasts[j] + 1, lasts[j] + 1 + rng.integers(0, 30)
        elif kind == 1:  # touching in front of j
            lasts[i] = firsts[j] - 1
            firsts[i] = lasts[i] - rng.integers(0, 30)
        elif kind == 2:  # identical
            firsts[i], lasts[i] = firsts[j], lasts[j]
        elif kind == 3:  # nested
            firsts[i] = rng.integers(firsts[j], lasts[j] + 1)
            lasts[i] = rng.integers(firsts[i], lasts[j] + 1)
    shift = max(0, -int(firsts.min()))
    return firsts + shift, lasts + shift


# ---- synthetic records ---------------------------------------------------------------------------------------------------
def metadata(norm_scale: float = 1.0, read_length: int = 50) -> dict:
    return {"read_length": read_length, "resolved_extend_bp": -1, "paired_end_mode": False, "norm_scale": float(norm_scale)}


def bin_reads(bins, seed: int, step: int = STEP, depth: int = 3, mapq: int = 30):
    """The six arrays of reads that cover exactly the bins ``bins`` (ascending) at ``step``: per bin 1 .. depth reads of one
    step's length that begin on the bin's first base, either strand.  The first and the last bin are covered, so the
    support is [bins[0], bins[-1]]."""
    rng = np.random.default_rng(seed)
    bins = np.asarray(bins, dtype=np.int64)
    copies = rng.integers(1, depth + 1, size=bins.size)
    pos = np.repeat(bins * step, copies).astype(np.int32)
    n = pos.size
    flag = np.where(rng.random(n) < 0.5, 0, 16).astype(np.uint16)
    return [pos, (pos + step).astype(np.int32), np.zeros(n, np.int32), flag, np.full(n, mapq, np.uint8), np.ones(n, np.uint8)]


def sparse_bins(first: int, last: int, seed: int, keep: float = 0.5) -> np.ndarray:
    """Ascending bins of [first, last] with both ends kept and about ``keep`` of those between."""
    rng = np.random.default_rng(seed)
    inner = np.arange(first + 1, last)
    return np.concatenate([[first], inner[rng.random(inner.size) < keep], [last]] if last > first else [[first]]).astype(np.int64)


def empty_records():
    return [np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint16), np.zeros(0, np.uint8),
            np.zeros(0, np.uint8)]


def second_turn_columns(shape: dict, rows: int = 3) -> int:
    """The number of columns at which ``rows`` rows of float64 take the fill kernel just past cap x unit elements: some
    workgroups write a second unit, the others one (asserted from the caps alone)."""
    unit, cap = shape["unit"], shape["max_grid"]
    m = (cap // rows + 5) * unit + 77
    units_per_row = -(-(m + 1) // unit)  # (a float64 row may start 8 bytes behind a 16-byte boundary: one more element)
    second_turn(rows * units_per_row * unit - 1, unit, cap)
    assert units_per_row * (rows - 1) < cap < units_per_row * rows, "the second turn does not begin inside the last row"
    return m
