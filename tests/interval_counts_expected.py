"""The arithmetic of row f6 (decoded alignment records -> one count per interval and file) stated in NumPy: one interval
of the reference's ``count_alignment_intervals`` is ``ccounts_countRegion`` over region = [start, end) with
intervalSizeBP = end - start and a buffer of one float, i.e. `alignment_counts_expected.count_region` with
``step = end - start`` and ``length = 1``.  tests/test_interval_counts_host.py pins this to
tests/golden/interval_count_vectors.npz, which the reference's compiled counter wrote; the GPU tests then compare the
kernels with it on random records."""
import json
import os

import numpy as np

import alignment_counts_expected as expected

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("pos", "end", "isize", "flag", "mapq", "mate_same")


def load_golden():
    arrays = np.load(os.path.join(GOLDEN, "interval_count_vectors.npz"))
    with open(os.path.join(GOLDEN, "interval_count_vectors.json"), encoding="utf-8") as handle:
        return arrays, json.load(handle)


def fields_of(arrays, key, contig):
    return tuple(arrays[f"f_{key}_{contig}_{field}"] for field in FIELDS)


def count_interval(fields, start, end, read_length=0, **options):
    """The integer the reference's float holds for one interval (below 2**24)."""
    return int(expected.count_region(*fields, int(start), int(end), int(end) - int(start), int(read_length), length=1, **options)[0])


def count_intervals(fields, starts, ends, read_length=0, **options):
    """int64 counts of the intervals over one track.  The records are cut to those whose pos lies in the interval's reach
    before the statement runs (it is O(records) per interval): a record with pos >= end or pos + span <= start is never
    yielded by the index iterator, which the statement tests again itself."""
    pos, end = np.asarray(fields[0], dtype=np.int64), np.asarray(fields[1], dtype=np.int64)
    out = np.zeros(len(starts), dtype=np.int64)
    if pos.size == 0:
        return out
    reach = np.maximum(end, pos + 1)
    for i, (s, e) in enumerate(zip(starts, ends)):
        keep = (pos < int(e)) & (reach > int(s))
        out[i] = count_interval(tuple(np.asarray(f)[keep] for f in fields), s, e, read_length, **options)
    return out


def count_matrix(fields_by_file, contigs, starts, ends, read_length=0, **options):
    """int64 [P, F]: ``fields_by_file[f][contig]`` are the six arrays of file f on that contig."""
    contigs = np.asarray(contigs)
    out = np.zeros((len(starts), len(fields_by_file)), dtype=np.int64)
    for f, by_contig in enumerate(fields_by_file):
        for contig in dict.fromkeys(contigs.tolist()):
            rows = np.flatnonzero(contigs == contig)
            out[rows, f] = count_intervals(by_contig[contig], np.asarray(starts)[rows], np.asarray(ends)[rows], read_length, **options)
    return out
