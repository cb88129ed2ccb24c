#!/usr/bin/env python3
"""Times row f12 (post-hoc scoring over BAM paths, rocco_amd/scores.py over rocco_amd/csrc/interval_count.hip).

    python tests/tools/score_paths_bench.py [--files 8] [--records 60000] [--peaks 4000] [--reps 5] > profiles/score_paths_bench.txt

Input: K synthetic coordinate-sorted BAM files with ``.bai`` indexes, written by the tests' own writers
(tests/bam_expected.py, tests/bam_index_files.py): three contigs, ``--records`` 50 bp records per file, a peak file of
``--peaks`` intervals of 200-2 000 bp.  Timed, host clock with a device synchronisation on either side, 1 warm-up +
``reps`` repetitions, the median:

  score_peaks        the whole function (facts, one counting pass over peaks and nulls, scoring, both files written);
                     the decoded contigs stay in the alignment cache between repetitions
  one-call pass      `_count_paths` alone: per contig group ONE rocco_hip_count_alignment_intervals_sets call, counts
                     stored at their final rows
  two-call pass      the same pass made of what the package had before: per contig group two
                     rocco_hip_count_alignment_intervals_batch calls (peaks, nulls), each into a dense temporary that
                     torch scatters into the result

Both passes are run at the default `GROUP_BYTES` (one group) and with one contig per group.  The two results must be equal
(exit 1 otherwise).  There is no bar: the numbers are recorded (DESIGN.md note (33))."""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CONTIGS = [("chr1", 3_000_000), ("chr2", 2_000_000), ("chrX", 1_000_000)]


def write_bam(np, bx, bif, folder, k, records):
    rng = np.random.default_rng(100 + k)
    body = []
    for tid, (_, length) in enumerate(CONTIGS):
        n = records * length // sum(size for _, size in CONTIGS)
        pos = np.sort(rng.integers(0, length - 100, size=n))
        flags = np.where(rng.random(n) < 0.5, 16, 0) | np.where(rng.random(n) < 0.03, 256, 0)
        mapq = rng.integers(0, 61, size=n)
        body += [bx.make_record(56, tid=tid, pos=int(p), flag=int(f), mapq=int(q), name=b"r\0", cigar=((0, 50),))
                 for p, f, q in zip(pos, flags, mapq)]
    raw = bx.bgzf_compress(bx.make_header(CONTIGS) + b"".join(body))
    return bif.write_pair(folder, f"sample{k}", raw)


def two_call_pass(torch, np, scores, readtracks, bam, files, families):
    """`scores._count_paths` with the existing entry point: per group one call per family, each scattered into the result."""
    chroms = [c for family in families for c in family[0]]
    out = torch.empty((len(chroms), len(files)), dtype=torch.int32, device="cuda:0")
    order = {name: k for k, (name, _) in enumerate(files[0].contigs)}
    wanted = sorted(dict.fromkeys(chroms), key=lambda c: order[c])
    costs = [20 * sum(f.count(c) for f in files) for c in wanted]
    for group in scores._contig_groups(wanted, costs, int(scores.GROUP_BYTES)):
        tracks = iter(bam._load_contigs([(f, c) for f in files for c in group]))
        records = [{c: next(tracks) for c in group} for _ in files]
        first = 0
        for family_chroms, starts, ends, options in families:
            rows = np.flatnonzero(np.isin(np.asarray(family_chroms, dtype=object), group))
            if rows.size:
                dense = readtracks.count_alignment_intervals_batch_device(
                    records, [family_chroms[i] for i in rows], np.asarray(starts)[rows], np.asarray(ends)[rows], **options)
                out[torch.from_numpy(rows + first).to(out.device)] = dense
            first += len(family_chroms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--records", type=int, default=60000)
    ap.add_argument("--peaks", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    import bam_expected as bx
    import bam_index_files as bif
    from rocco_amd import bam, readtracks, scores

    assert torch.cuda.is_available(), "this tool measures on the GPU only"

    def timed(call):
        times = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return result, statistics.median(times[1:]) * 1e3

    with tempfile.TemporaryDirectory(prefix="score_paths_bench_") as folder:
        paths = [write_bam(np, bx, bif, folder, k, args.records) for k in range(args.files)]
        sizes, peaks = os.path.join(folder, "g.sizes"), os.path.join(folder, "peaks.bed")
        with open(sizes, "w") as handle:
            handle.write("".join(f"{name}\t{length}\n" for name, length in CONTIGS))
        rng = np.random.default_rng(7)
        rows = []
        for _ in range(args.peaks):
            name, length = CONTIGS[int(rng.integers(0, len(CONTIGS)))]
            width = int(rng.integers(200, 2001))
            start = int(rng.integers(0, length - width))
            rows.append((name, start, start + width))
        with open(peaks, "w") as handle:
            handle.write("".join(f"{c}\t{s}\t{e}\n" for c, s, e in sorted(rows)))
        print(f"device {torch.cuda.get_device_name(0)}; {args.files} files of {args.records} records over {len(CONTIGS)} contigs, "
              f"{args.peaks} peaks, {args.reps} repetitions (median, ms)")

        def whole():
            matrix = os.path.join(folder, "bench.counts.tsv")
            if os.path.exists(matrix):
                os.remove(matrix)
            return scores.score_peaks(paths, sizes, peaks, count_matrix_file=matrix, output_file=os.path.join(folder, "bench.narrowPeak"),
                                      skip_for_norm=["chrX"], ecdf_nsamples=500, seed=11)

        _, ms = timed(whole)
        print(f"score_peaks, whole function: {ms:.2f} ms")
        files = [bam._cached_file(p) for p in paths]
        chroms, starts, ends, _, _ = scores._read_peak_intervals(peaks)
        lengths = np.asarray([e - s for s, e in zip(starts, ends)], dtype=np.float64)
        _, bins = scores._assign_length_bins(lengths)
        _, per_length = scores._null_intervals(bins, sizes, 500, 11)
        families = [scores._peak_family(chroms, starts, ends), scores._null_family([i for group in per_length for i in group])]
        print(f"counting pass: {len(chroms)} peaks + {len(families[1][0])} null regions ({len(bins)} length bins)")
        failed = False
        for label, budget in (("one group", scores.GROUP_BYTES), ("one contig per group", 1)):
            scores.GROUP_BYTES = budget
            one, one_ms = timed(lambda: scores._count_paths(files, families))
            two, two_ms = timed(lambda: two_call_pass(torch, np, scores, readtracks, bam, files, families))
            same = bool(torch.equal(one, two))
            failed |= not same
            print(f"{label}: one-call pass {one_ms:.2f} ms, two-call pass {two_ms:.2f} ms, ratio {two_ms / one_ms:.2f}, equal {same}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
