"""Times score_dispersion_chrom_device on hg38 chr1 in 50 bp bins (K = 100 x 4 979 129, float64; 3.98 GB), against the
median launch and against the MAD a caller could compose before the fused kernel existed:

    python scripts/bench_dispersion.py [--n N] [--K K] [--dtype f64|f32]

  (a) median      score_central_tendency_chrom_device                               reads 8 K n
  (b) composed    median -> (m - median).abs_() in torch -> median                  reads 8 K n four times, writes it twice
  (c) mad, iqr, std, tstd  one fused launch each                                    reads 8 K n

3 warm-ups and 10 repetitions of each, every repetition between two HIP events; the median and the minimum are printed,
with the algorithmic bytes over the median time.  `--n` small enough for the 256 MiB Infinity Cache shows the kernels
without HBM traffic (compute bound).

The one condition: the fused `mad` (c) must not take longer than the composition (b), median against median.  The script
exits with status 1 when it does, and when the two disagree in a single bit.  The recorded run is
profiles/dispersion_bench.txt."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rocco_amd import rocco as rr, synth  # noqa: E402

WARMUPS, REPS = 3, 10


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
    ap.add_argument("--n", type=int, default=4979129)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    args = ap.parse_args()
    K, n = args.K, args.n
    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    m = synth.hash_matrix_device(K, n, synth.chrom_seed(20240, 0), dtype=dtype)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    matrix_bytes = m.element_size() * K * n
    print(f"K = {K}, n = {n}, {args.dtype}: matrix {matrix_bytes / 1e9:.3f} GB on {torch.cuda.get_device_name(0)}; "
          f"{WARMUPS} warm-ups, {REPS} repetitions, HIP events")

    def composed():
        med = rr.score_central_tendency_chrom_device(m)
        return rr.score_central_tendency_chrom_device((m - med).abs_(), out)

    rows = [
        ("(a) median", lambda: rr.score_central_tendency_chrom_device(m, out), matrix_bytes + 8 * n),
        # reads: median, subtraction, abs_, second median; writes: the K x n temporary twice, two score vectors
        ("(b) composed mad", composed, 6 * matrix_bytes + 16 * n),
        ("(c) mad", lambda: rr.score_dispersion_chrom_device(m, out, method="mad"), matrix_bytes + 8 * n),
        ("(c) iqr 25-75", lambda: rr.score_dispersion_chrom_device(m, out, method="iqr"), matrix_bytes + 8 * n),
        ("(c) std", lambda: rr.score_dispersion_chrom_device(m, out, method="std"), matrix_bytes + 8 * n),
        ("(c) tstd 0.05", lambda: rr.score_dispersion_chrom_device(m, out, method="tstd"), matrix_bytes + 8 * n),
    ]
    results = {}
    for name, fn, moved in rows:
        med_ms, min_ms = timed(fn)
        results[name] = med_ms
        print(f"{name:<18} median {med_ms:9.3f} ms   min {min_ms:9.3f} ms   {moved / 1e9:7.3f} GB algorithmic   "
              f"{moved / med_ms / 1e9:6.2f} TB/s   x{med_ms / results['(a) median']:5.2f} of (a)")
    fused, parent = results["(c) mad"], results["(b) composed mad"]
    print(f"fused mad / composed mad = {fused / parent:.3f}")
    failed = False
    if fused > parent:
        print(f"FAIL: fused mad ({fused:.3f} ms) is slower than the composition ({parent:.3f} ms)")
        failed = True
    if torch.equal(rr.score_dispersion_chrom_device(m, method="mad"), composed()):
        print("fused mad == composed mad, bit for bit")
    else:
        print("FAIL: fused mad != composed mad")
        failed = True
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
