"""The arithmetic of row f5 (decoded alignment records -> binned coverage) stated in NumPy, for inputs larger than
the fixtures.  tests/test_alignment_counts_host.py pins every function here to tests/golden/alignment_count_vectors.npz,
which the reference's compiled counter and its own ``get_bam_chrom_reads`` wrote; the GPU tests then compare the
kernels with these functions on random records.

Records are six arrays in file order: pos, end (bam_endpos), isize, flag, mapq, mate_same."""
import logging

import numpy as np

PROPER_PAIR, MATE_UNMAPPED, REVERSE, READ2 = 2, 8, 16, 128
TAIL_CUSHION = 2_000_000
logger = logging.getLogger(__name__)


def n_bins(start, end, step):
    return (end - start - 1) // step + 1


def _c_div(a, b):
    """C's integer division (towards zero) of int64 arrays by a positive b."""
    return np.where(a >= 0, a // b, -((-a) // b))


def difference_cells(pos, end, isize, flag, mapq, mate_same, start, stop, step, read_length, one_read_per_bin=0, flag_include=0,
                     flag_exclude=0, shift_forward_strand53=0, shift_reverse_strand53=0, extend_bp=0, max_insert_size=1000,
                     paired_end_mode=0, min_mapping_quality=0, min_template_length=-1, length=None):
    """int64 cells, ``length`` + 1 of them (default: the bins of [start, stop)): +1 where a fragment begins and -1 behind
    its last bin (the last cell lies behind the last bin), or the counts themselves with one_read_per_bin."""
    pos, end, isize = (np.asarray(a, dtype=np.int64) for a in (pos, end, isize))
    flag, mapq = np.asarray(flag, dtype=np.int64), np.asarray(mapq, dtype=np.int64)
    mate_same = np.asarray(mate_same, dtype=np.int64) != 0
    length = n_bins(start, stop, step) if length is None else int(length)
    flag_include, flag_exclude = max(flag_include, 0) & 0xFFFF, max(flag_exclude, 0) & 0xFFFF
    # what the index iterator yields: the read as it lies in the file overlaps the region
    keep = (pos < stop) & (np.maximum(end, pos + 1) > start)
    if flag_include > 0:
        keep &= (flag & flag_include) == flag_include
    keep &= (flag & flag_exclude) == 0
    keep &= mapq >= min_mapping_quality
    forward = (flag & REVERSE) == 0
    shift = np.where(forward, shift_forward_strand53, -shift_reverse_strand53)
    if paired_end_mode > 0:
        template = np.abs(isize)
        least = min_template_length if min_template_length >= 0 else read_length
        keep &= ((flag & PROPER_PAIR) != 0) & ((flag & READ2) == 0) & ((flag & MATE_UNMAPPED) == 0) & mate_same
        keep &= (template != 0) & (template >= least)
        if max_insert_size > 0:
            keep &= template <= max_insert_size
        lo = np.where(isize >= 0, pos, end - template) + shift
        hi = lo + template
    elif extend_bp > 0:
        lo = np.where(forward, pos + shift, end + shift - extend_bp)
        hi = lo + extend_bp
    else:
        lo, hi = pos + shift, end + shift
    keep &= (hi > start) & (lo < stop)
    lo, hi = np.clip(lo[keep], start, None), np.clip(hi[keep], None, stop)
    cells = np.zeros(length + 1, dtype=np.int64)
    if one_read_per_bin:
        index = _c_div((lo + hi) // 2 - start, step).astype(np.uint64)
        index = index[index < np.uint64(length)].astype(np.int64)
        np.add.at(cells, index, 1)
    else:
        index0 = _c_div(lo - start, step).astype(np.uint64)
        index1 = _c_div(hi - 1 - start, step).astype(np.uint64)
        index1 = np.minimum(index1, np.uint64(length - 1))
        ok = (index0 < np.uint64(length)) & (index0 <= index1)
        np.add.at(cells, index0[ok].astype(np.int64), 1)
        np.add.at(cells, index1[ok].astype(np.int64) + 1, -1)
    return cells


def count_region(pos, end, isize, flag, mapq, mate_same, start, stop, step, read_length, into=None, **options):
    """float32 counts of the ``length`` bins (default: the bins of [start, stop)), added to ``into`` when given."""
    cells = difference_cells(pos, end, isize, flag, mapq, mate_same, start, stop, step, read_length, **options)
    counts = cells[:-1] if options.get("one_read_per_bin") else np.cumsum(cells[:-1])
    counts = counts.astype(np.float32)
    return counts if into is None else (np.asarray(into, dtype=np.float32) + counts).astype(np.float32)


def max_magnitude(pos, end, isize, flag, mapq, mate_same, start, stop, step, read_length, **options):
    """What the 2**24 condition is about: the largest magnitude among the difference cells (the one behind the last bin
    included) and the running values; with one_read_per_bin the largest count."""
    cells = difference_cells(pos, end, isize, flag, mapq, mate_same, start, stop, step, read_length, **options)
    if options.get("one_read_per_bin"):
        return int(np.max(np.abs(cells[:-1]), initial=0))
    return int(max(np.max(np.abs(cells), initial=0), np.max(np.abs(np.cumsum(cells[:-1])), initial=0)))


def chrom_range(pos, end, flag, chrom_size, flag_exclude):
    """(start, end): pos of the first record flag_exclude passes; end of the LAST one, in file order, among the records
    that reach into the last 2 Mb of the contig.  0 where there is none."""
    pos, end, flag = np.asarray(pos, dtype=np.int64), np.asarray(end, dtype=np.int64), np.asarray(flag, dtype=np.int64)
    passes = ((flag & max(flag_exclude, 0)) == 0) & (pos < chrom_size)
    reach = np.maximum(end, pos + 1)
    head = np.flatnonzero(passes & (reach > 0))
    tail = np.flatnonzero(passes & (reach > max(chrom_size - TAIL_CUSHION, 0)))
    return (int(pos[head[0]]) if head.size else 0), (int(end[tail[-1]]) if tail.size else 0)


def count_window(chrom_start, chrom_end, chrom_size, step):
    """The region get_bam_chrom_reads counts for a contig's range."""
    count_start = max(0, (chrom_start // step) * step)
    count_end = min(chrom_size, int(np.ceil(max(chrom_end, count_start + 1) / float(step)) * step))
    if count_end <= count_start:
        count_end = min(chrom_size, count_start + step)
    return count_start, count_end


def tail(counts, count_start, step, norm_scale, scale_by_step=False, const_scale=1.0, round_digits=5):
    """(intervals, values) or (None, None): scaling in float64, the positive support, np.round."""
    vals = np.asarray(counts, dtype=np.float64)
    intervals = count_start + np.arange(vals.size, dtype=np.int64) * int(step)
    vals = vals * float(norm_scale)
    if scale_by_step:
        vals = vals / float(step)
    if const_scale >= 0:
        vals = vals * const_scale
    positive = np.flatnonzero(vals > 0.0)
    if positive.size == 0:
        return None, None
    first, last = int(positive[0]), int(positive[-1]) + 1
    return intervals[first:last].astype(int), np.round(vals[first:last], round_digits)


def bam_chrom_reads(pos, end, isize, flag, mapq, mate_same, chrom_size, step, metadata, min_mapping_score=10, flag_include=None,
                    flag_exclude=3844, center_reads=False, const_scale=1.0, round_digits=5, scale_by_step=False):
    """Everything get_bam_chrom_reads does after the metadata lookup."""
    chrom_start, chrom_end = chrom_range(pos, end, flag, chrom_size, max(0, int(flag_exclude)))
    if chrom_end <= chrom_start:
        return None, None
    count_start, count_end = count_window(chrom_start, chrom_end, chrom_size, step)
    counts = count_region(pos, end, isize, flag, mapq, mate_same, count_start, count_end, int(step), int(metadata["read_length"]),
                          one_read_per_bin=1 if center_reads else 0, flag_include=max(0, int(flag_include or 0)),
                          flag_exclude=max(0, int(flag_exclude)), extend_bp=max(0, int(metadata["resolved_extend_bp"])),
                          paired_end_mode=1 if bool(metadata["paired_end_mode"]) else 0,
                          min_mapping_quality=max(0, int(min_mapping_score)))
    return tail(counts, count_start, step, metadata["norm_scale"], scale_by_step, const_scale, round_digits)


def random_records(rng, n, span, read=50, paired=0.5, first=0):
    """n position-sorted records over [first, first + span): both strands, pairs of either sign, odd flags, ragged ends."""
    pos = np.sort(rng.integers(first, first + span, size=n)).astype(np.int32)
    end = (pos + np.where(rng.random(n) < 0.1, rng.integers(1, 4 * read, size=n), read)).astype(np.int32)
    flag = np.where(rng.random(n) < 0.5, 0, 16).astype(np.int64)
    is_pair = rng.random(n) < paired
    flag |= np.where(is_pair, 1 | np.where(rng.random(n) < 0.85, 2, 0) | np.where(rng.random(n) < 0.5, 64, 128), 0)
    flag |= np.where(rng.random(n) < 0.03, 8, 0) | np.where(rng.random(n) < 0.03, 256, 0) | np.where(rng.random(n) < 0.03, 1024, 0)
    flag |= np.where(rng.random(n) < 0.02, 4, 0)
    isize = np.where(is_pair, rng.integers(-700, 700, size=n), 0).astype(np.int32)
    mapq = rng.integers(0, 61, size=n).astype(np.uint8)
    mate_same = (rng.random(n) < 0.95).astype(np.uint8)
    return pos, end, isize, flag.astype(np.uint16), mapq, mate_same
