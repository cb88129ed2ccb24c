#!/usr/bin/env python3
"""Times row f6 (decoded alignment records -> one count per interval and file, rocco_amd/csrc/interval_count.hip) at the
size of a chr1 track.

    python tests/tools/interval_count_bench.py [--records 20000000] [--files 1 8] [--reps 10] > profiles/interval_count_bench.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/interval_count_bench.py --reps 3 --files 1 --no-compare

Input: F files of one synthetic track each, N position-sorted records of 50 bp over 248 Mb; 50 000 peaks of 200-2 000 bp
plus 24 x 500 null regions (24 lengths, 500 random regions each), all in one call at raw_count_matrix's options.
Timing: HIP events around the library's entry point (three kernels, the scan, two small copies; the records are in HBM
before, the counts are in HBM after), 3 warm-ups + `reps` repetitions, the median.  Reported: that time, the bytes of the
candidates the counting kernel reads (16 B each) and the rate they make.

Comparison: the only route the package had before, one `count_alignment_region_from_records` call per interval (each
streams all N records), on the first 256 peaks of the first file, against the new call on the same 256, host clock,
records on the device in both.  Exits 1 if the new call is slower or any count differs."""
import argparse
import ctypes
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SPAN, READ = 248_000_000, 50
RAW = dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10)


def synthetic_track(torch, n, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    pos = torch.sort(torch.randint(0, SPAN - 1000, (n,), generator=g, device=device, dtype=torch.int64)).values.to(torch.int32)
    flag = (torch.randint(0, 2, (n,), generator=g, device=device, dtype=torch.int32) * 16).to(torch.int16)
    mapq = torch.randint(0, 61, (n,), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
    return pos, pos + READ, torch.zeros(n, dtype=torch.int32, device=device), flag, mapq, torch.ones(n, dtype=torch.uint8, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--files", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--peaks", type=int, default=50_000)
    ap.add_argument("--compare", type=int, default=256)
    ap.add_argument("--no-compare", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from rocco_amd import _native
    from rocco_amd import dp as _dp
    from rocco_amd.readtracks import (AlignmentRecords, CountOptions, _count_options, count_alignment_intervals_batch_device,
                                      count_alignment_region_from_records, count_intervals_shape)

    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda:0")
    lib, solver = _native.load(), _native.solver_for(0)
    rng = np.random.default_rng(17)
    widths = np.concatenate([rng.integers(200, 2001, size=args.peaks), np.repeat(np.unique(rng.integers(150, 5000, size=200))[:24], 500)])
    starts_h = rng.integers(0, SPAN - 6000, size=widths.size).astype(np.int32)
    ends_h = (starts_h + widths).astype(np.int32)
    P = int(widths.size)
    ids_t = torch.zeros(P, dtype=torch.int32, device=dev)
    starts_t, ends_t = torch.from_numpy(starts_h).to(dev), torch.from_numpy(ends_h).to(dev)
    print(f"device {torch.cuda.get_device_name(0)}; {args.records} records per file, {P} intervals ({args.peaks} peaks of 200-2000 bp, "
          f"{P - args.peaks} null regions); shape {count_intervals_shape()}")
    failed = False
    first_track = None
    for F in args.files:
        tracks = [synthetic_track(torch, args.records, 100 + f, dev) for f in range(F)]
        if first_track is None:
            first_track = tracks[0]
        cat = [torch.cat([t[i] for t in tracks]) if F > 1 else tracks[0][i] for i in range(6)]
        candidates = 0
        for t in tracks:  # every record spans READ: the candidates of an interval are the records with start - READ < pos < end
            pos64 = t[0].to(torch.int64)
            lo = torch.searchsorted(pos64, (starts_t.to(torch.int64) - READ + 1), right=False)
            hi = torch.searchsorted(pos64, ends_t.to(torch.int64), right=False)
            candidates += int((hi - lo).sum())
            del pos64
        del tracks
        opts = _count_options(0, **RAW)
        rec_off = (ctypes.c_longlong * (F + 1))(*[f * args.records for f in range(F + 1)])
        facts = (ctypes.c_int * (2 * F))()
        out = torch.empty((P, F), dtype=torch.int32, device=dev)
        stream = _dp._stream_ptr(out)

        def run():
            rc = lib.rocco_hip_count_alignment_intervals_batch(solver.handle, *[c.data_ptr() for c in cat], rec_off, F, 1, ctypes.byref(opts),
                                                               ids_t.data_ptr(), starts_t.data_ptr(), ends_t.data_ptr(), P, out.data_ptr(),
                                                               facts, stream)
            assert rc == 0, rc

        times = []
        for rep in range(args.reps + 3):  # three warm-ups
            begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            begin.record()
            run()  # (ends in its own stream synchronise)
            done.record()
            done.synchronize()
            if rep >= 3:
                times.append(begin.elapsed_time(done) * 1e-3)
        med = statistics.median(times)
        assert all(facts[2 * f] == READ and facts[2 * f + 1] == 0 for f in range(F))
        print(f"F={F}: {int(out.sum())} reads counted, deepest interval {int(out.max())}; median {med * 1e3:8.3f} ms  min {min(times) * 1e3:8.3f}  "
              f"max {max(times) * 1e3:8.3f}  ({len(times)} calls); candidates {candidates} = {candidates * 16 / 1e6:.1f} MB read by the "
              f"counting kernel, {candidates * 16 / med / 1e9:.1f} GB/s; the facts pass reads {F * args.records * 8 / 1e6:.0f} MB more "
              f"({(candidates * 16 + F * args.records * 8) / med / 1e9:.1f} GB/s with it)")
        del cat, out
        torch.cuda.empty_cache()
    if not args.no_compare:
        n = min(args.compare, args.peaks)
        records = AlignmentRecords(*first_track)
        s, e = [int(v) for v in starts_h[:n]], [int(v) for v in ends_h[:n]]
        for _ in range(2):  # (the first round warms both routes up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old = np.array([count_alignment_region_from_records(records, s[i], e[i], e[i] - s[i], 0, **RAW)[0] for i in range(n)])
            t_old = time.perf_counter() - t0
            t0 = time.perf_counter()
            new = count_alignment_intervals_batch_device([{"chr1": records}], ["chr1"] * n, s, e, **RAW).cpu().numpy()[:, 0]
            t_new = time.perf_counter() - t0
        same = bool(np.array_equal(old.astype(np.int64), new.astype(np.int64)))
        print(f"first {n} peaks, one file: one region call per interval {t_old * 1e3:.1f} ms, one batched call {t_new * 1e3:.3f} ms "
              f"({t_old / t_new:.0f}x); counts {'equal' if same else 'DIFFER'}")
        failed = failed or not same or t_new > t_old
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
