#!/usr/bin/env python3
"""Times row f7 (decoded records of a whole file -> fragment length, rocco_amd/csrc/fragment_length.hip) at the size of a
single-end file's three longest contigs.

    python tests/tools/fragment_length_bench.py [--records 20000000] [--reps 5] [--blocks 4096] > profiles/fragment_length_bench.txt

Input: one synthetic single-end file made on the device: chr1 / chr2 / chr3-sized contigs (248, 242 and 198 Mb) with N
position-sorted 50-bp records shared among them by length, three quarters of them in 200 000 peaks of strand-shifted reads
(forward reads ~ N(centre - 90, 40), reverse reads ending ~ N(centre + 90, 40)), the rest uniform.
Timed with HIP events around each entry point (records in HBM before; every entry point ends in its own stream
synchronise), one warm-up + `reps` repetitions, the median:
  the mapped-count pass        rocco_hip_record_flag_facts: 6 B per record read (pos, flag)
  density + ranking + pick     rocco_hip_fragment_block_centers at the defaults with max_iterations = `blocks`: 6 B per record
                               read by the density pass (pos, flag); the window sums, the sort of ~2.75 M chunk sums and the
                               host pick come on top, so the GB/s of the record bytes is a lower bound on the density pass
  the cross-correlation        rocco_hip_strand_xcorr_blocks over the first `blocks` centres of chr1 at block_size 5 000,
                               lags 50, 55, .. 1 000
No speed bar: the only fair comparison is the reference's CPU routine, which does not travel to the GPU machine."""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
CONTIGS = [("chr1", 248_000_000), ("chr2", 242_000_000), ("chr3", 198_000_000)]
READ = 50


def synthetic_contig(torch, n, length, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    peaks = max(n // 100, 1)
    centres = torch.randint(2000, length - 2000, (peaks,), generator=g, device=device, dtype=torch.int64)
    in_peaks = (3 * n) // 4
    which = torch.randint(0, peaks, (in_peaks,), generator=g, device=device, dtype=torch.int64)
    reverse = torch.randint(0, 2, (n,), generator=g, device=device, dtype=torch.int64)
    jitter = (torch.randn(in_peaks, generator=g, device=device) * 40.0).to(torch.int64)
    five_prime = centres[which] + jitter + torch.where(reverse[:in_peaks] == 1, 90, -90)
    pos_peaks = torch.where(reverse[:in_peaks] == 1, five_prime - READ + 1, five_prime)
    pos = torch.cat([pos_peaks, torch.randint(0, length - READ, (n - in_peaks,), generator=g, device=device, dtype=torch.int64)])
    pos = pos.clamp_(0, length - READ)
    pos, order = torch.sort(pos)
    flag = (reverse[order] * 16).to(torch.int16)
    pos = pos.to(torch.int32)
    zeros = torch.zeros(n, dtype=torch.int32, device=device)
    return pos, pos + READ, zeros, flag, torch.full((n,), 30, dtype=torch.uint8, device=device), torch.zeros(n, dtype=torch.uint8, device=device)


def timed(torch, call, reps):
    times = []
    for rep in range(reps + 1):  # one warm-up
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        result = call()
        done.record()
        done.synchronize()
        if rep >= 1:
            times.append(begin.elapsed_time(done) * 1e-3)
    return statistics.median(times), min(times), max(times), result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4096)
    args = ap.parse_args()
    import torch

    from rocco_amd.readtracks import (AlignmentFileRecords, AlignmentRecords, _block_starts, _records_on_device,
                                      alignment_fragment_length_from_records, fragment_block_centers_device, fragment_length_shape,
                                      record_flag_facts_device, strand_xcorr_blocks_device)

    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda:0")
    total = sum(length for _, length in CONTIGS)
    records = {}
    for k, (name, length) in enumerate(CONTIGS):
        n = args.records * length // total
        fields = synthetic_contig(torch, n, length, 40 + k, dev)
        records[name] = AlignmentRecords(*fields, qlen=torch.full((n,), READ, dtype=torch.int32, device=dev))
    tracks = [records[name] for name, _ in CONTIGS]
    lengths = [length for _, length in CONTIGS]
    cat, offsets = _records_on_device(tracks, dev)
    n_records = int(offsets[-1])
    print(f"device {torch.cuda.get_device_name(0)}; {n_records} records over {[n for n, _ in CONTIGS]}; shape {fragment_length_shape()}")

    med, low, high, (mapped, unsorted) = timed(torch, lambda: record_flag_facts_device(tracks, cat, offsets), args.reps)
    assert sum(mapped) == n_records and not any(unsorted)
    print(f"mapped-count pass: median {med * 1e3:8.3f} ms  min {low * 1e3:8.3f}  max {high * 1e3:8.3f}; {n_records * 6 / 1e6:.0f} MB of "
          f"records read, {n_records * 6 / med / 1e9:.1f} GB/s")

    med, low, high, centers = timed(torch, lambda: fragment_block_centers_device(tracks, lengths, 0, args.blocks, 5000, 250, cat=cat,
                                                                                offsets=offsets), args.reps)
    chunks = sum((length + 249) // 250 for length in lengths)
    print(f"density + ranking + pick: median {med * 1e3:8.3f} ms  min {low * 1e3:8.3f}  max {high * 1e3:8.3f}; {chunks} chunk sums ranked, "
          f"{[int(c.size) for c in centers]} centres; {n_records * 6 / 1e6:.0f} MB of records read by the density pass, "
          f"{n_records * 6 / med / 1e9:.1f} GB/s of them over the whole step (a lower bound on the density pass)")

    starts = _block_starts(centers[0], lengths[0], 5000, 250)[: args.blocks]
    block_track = [0] * int(starts.size)
    med, low, high, (best_lag, best_score, _, _) = timed(
        torch, lambda: strand_xcorr_blocks_device(tracks, block_track, starts.tolist(), [READ, READ, READ], 0, 5000, 1000, 5, cat=cat,
                                                  offsets=offsets), args.reps)
    candidates = int(((best_lag > 0) & (best_score != 0.0)).sum())
    lags = (1000 - READ) // 5 + 1
    additions = sum(5000 - (READ + 5 * j) for j in range(lags)) * int(starts.size)
    print(f"cross-correlation of {int(starts.size)} blocks x {lags} lags: median {med * 1e3:8.3f} ms  min {low * 1e3:8.3f}  max {high * 1e3:8.3f}; "
          f"{candidates} candidates; {additions / 1e9:.2f} G dependent multiply-adds, {additions / med / 1e9:.1f} G/s")

    file = AlignmentFileRecords(CONTIGS, records, name="synthetic")
    med, low, high, length = timed(torch, lambda: alignment_fragment_length_from_records(file, max_iterations=4096), args.reps)
    print(f"alignment_fragment_length_from_records(max_iterations=4096), end to end: median {med * 1e3:8.3f} ms  min {low * 1e3:8.3f}  "
          f"max {high * 1e3:8.3f}; fragment length {length}")


if __name__ == "__main__":
    main()
