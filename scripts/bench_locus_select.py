"""Times the ten default score quantiles of a genome's 24 score vectors (hg38 in 50 bp bins, 61 765 409 loci), by the
batched radix select against one radix sort per chromosome:

    python scripts/bench_locus_select.py [--step BP] [--K K]

  (a) select   ONE cscores_quantiles_batch_device call for all 24 vectors          reads 8 n per pass, six passes
  (b) sort     budget.sort_device + budget.sorted_probe per chromosome             a 64-bit radix sort: at least 8 passes
                                                                                   x 16 bytes per value (the path the
                                                                                   budget estimate takes)

Input 1: the scores are the medians of K = 10 hash tracks (rocco_amd.synth); input 2: the same with 90 % of the loci set
to 0.  3 warm-ups and 10 repetitions of each, every repetition between two HIP events; the median and the minimum are
printed, with the algorithmic bytes over the median time.

The one condition, on both inputs: (a) must not take longer than (b), median against median, and the two must agree in
every bit.  The script exits with status 1 otherwise.  The recorded run is profiles/locus_select_bench.txt."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rocco_amd import budget, rocco as rr, synth  # noqa: E402

WARMUPS, REPS = 3, 10
SELECT_PASSES = 6  # csrc/select.hip: every pass reads every value


def timed(fn):
    for _ in range(WARMUPS):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        fn()
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))  # ms
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=50)
    ap.add_argument("--K", type=int, default=10)
    args = ap.parse_args()
    loci = synth.chrom_loci(args.step)
    total = sum(n for _, n in loci)
    scores = [rr.score_central_tendency_chrom_device(synth.hash_matrix_device(args.K, n, synth.chrom_seed(20240, i)))
              for i, (_, n) in enumerate(loci)]
    gen = torch.Generator(device="cuda:0").manual_seed(90)
    sparse = [torch.where(torch.rand(s.shape[0], device=s.device, generator=gen) < 0.9, torch.zeros_like(s), s) for s in scores]
    print(f"{len(loci)} chromosomes, {total} loci at {args.step} bp, medians of K = {args.K} hash tracks on "
          f"{torch.cuda.get_device_name(0)}; {WARMUPS} warm-ups, {REPS} repetitions, HIP events")
    ranks = [[rr._higher_quantile_rank(int(s.shape[0]), q) for q in rr._DEFAULT_QUANTILES] for s in scores]

    def by_sort(vectors):
        rows = []
        for v, r in zip(vectors, ranks):
            ordered = budget.sort_device(v)
            rows.append(budget.sorted_probe(ordered, ranks=r[:8])[0] + budget.sorted_probe(ordered, ranks=r[8:])[0])
        return rows

    failed = False
    for label, vectors in (("hash-track medians", scores), ("the same, 90 % of the loci set to 0", sparse)):
        zeros = sum(int((v == 0).sum()) for v in vectors)
        print(f"input: {label} ({100.0 * zeros / total:.1f} % exact zeros)")
        select_ms, select_min = timed(lambda: rr.cscores_quantiles_batch_device(vectors))
        sort_ms, sort_min = timed(lambda: by_sort(vectors))
        for name, med_ms, min_ms, moved in (("(a) select, one call", select_ms, select_min, SELECT_PASSES * 8 * total),
                                            ("(b) sort + probe per chromosome", sort_ms, sort_min, 128 * total)):
            print(f"  {name:<32} median {med_ms:9.3f} ms   min {min_ms:9.3f} ms   {moved / 1e9:6.3f} GB algorithmic"
                  f"{' (at least)' if moved == 128 * total else '           '}   {moved / med_ms / 1e9:6.2f} TB/s")
        print(f"  select / sort = {select_ms / sort_ms:.4f}   (sort / select = {sort_ms / select_ms:.1f})")
        if select_ms > sort_ms:
            print(f"  FAIL: the select ({select_ms:.3f} ms) is slower than the sorts ({sort_ms:.3f} ms)")
            failed = True
        got = rr.cscores_quantiles_batch_device(vectors).cpu().numpy()
        want = np.array(by_sort(vectors), dtype=np.float64)
        if got.tobytes() == want.tobytes():
            print("  select == sort, bit for bit")
        else:
            print(f"  FAIL: select != sort in {int((got.view(np.uint64) != want.view(np.uint64)).sum())} of {got.size} values")
            failed = True
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
