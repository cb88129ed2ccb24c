#!/usr/bin/env python3
"""Times row f9 (K decoded files of one chromosome -> its count matrix in one device pass, rocco_amd/csrc/track_matrix.hip and
the batch kernels of count.hip) against the route the package had before, at the size of chr1.

    python tests/tools/bam_matrix_bench.py [--records 2000000] [--tracks 8 32] [--reps 5] > profiles/bam_matrix_bench.txt

Input: K synthetic tracks of N position-sorted single-end records of 50 bp over chr1 (248 956 422 bp), step 50, made on
the device from a seed; the records are in HBM before either route starts.
New route: `rocco_amd.readtracks.bam_chrom_matrix_from_records_batch` (starts on the host, matrix in HBM).
Old route: `bam_chrom_reads_from_records_batch`, then `assemble_chrom_matrix_device`, then what the composed driver did with
the NumPy return of `readtracks.generate_chrom_matrix`: the result copied to the host and `rocco._matrix_to_device` applied.
Both run in this process, one after the other per repetition; one warm-up of each, then `reps` repetitions; HIP events
around each call and the host clock; medians, and the old route's spread (max - min) between repetitions.  The results of
the two routes are compared bit for bit once per K.
Then the fill kernel alone (`rocco_hip_track_matrix_fill` over K full rows and one segment): HIP events, the median, and
the bytes per second it makes at 4 B read + 8 B written per element.
Exits 1 if the results differ or the new route's median is slower than the old one's by more than the old route's spread."""
import argparse
import ctypes
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
CHR1, STEP, READ = 248_956_422, 50, 50


def synthetic_track(torch, n, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    pos = torch.sort(torch.randint(10_000, CHR1 - 10_000, (n,), generator=g, device=device, dtype=torch.int64)).values.to(torch.int32)
    flag = (torch.randint(0, 2, (n,), generator=g, device=device, dtype=torch.int32) * 16).to(torch.int16)
    mapq = torch.randint(10, 61, (n,), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
    return pos, pos + READ, torch.zeros(n, dtype=torch.int32, device=device), flag, mapq, torch.ones(n, dtype=torch.uint8, device=device)


def timed(torch, call):
    begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    begin.record()
    result = call()
    done.record()
    done.synchronize()
    return result, begin.elapsed_time(done) * 1e-3, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--tracks", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import logging

    import numpy as np
    import torch

    from rocco_amd import _native
    from rocco_amd import dp as _dp
    from rocco_amd import readtracks as rt
    from rocco_amd import rocco as rr

    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    rt.logger.setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    lib, solver = _native.load(), _native.solver_for(0)
    print(f"device {torch.cuda.get_device_name(0)}; chr1 = {CHR1} bp at step {STEP}, {args.records} records per track; shape {rt.track_matrix_shape()}")
    failed = False
    for K in args.tracks:
        records = [rt.AlignmentRecords._of(*synthetic_track(torch, args.records, 300 + k, dev)) for k in range(K)]
        metas = [{"read_length": READ, "resolved_extend_bp": -1, "paired_end_mode": False, "norm_scale": 1.0 + 0.01 * k} for k in range(K)]

        def new_route():
            return rt.bam_chrom_matrix_from_records_batch(records, CHR1, STEP, metas)

        def old_route():
            intervals, vals = rt.bam_chrom_reads_from_records_batch(records, CHR1, STEP, metas)
            common_t, matrix_t = rt.assemble_chrom_matrix_device(intervals, vals)
            starts, matrix = common_t.cpu().numpy().astype(int), matrix_t.cpu().numpy()  # (the return of readtracks.generate_chrom_matrix)
            return starts, rr._matrix_to_device(matrix)

        rows = {"new": ([], []), "old": ([], [])}
        for rep in range(args.reps + 1):  # one warm-up
            for name, route in (("old", old_route), ("new", new_route)):
                (starts, matrix), device_s, wall_s = timed(torch, route)
                if rep == 0:
                    if name == "old":
                        want = (starts, matrix)
                    else:
                        same = bool(np.array_equal(starts, want[0])) and matrix.shape == want[1].shape and \
                            bool(torch.equal(matrix.view(torch.int64), want[1].view(torch.int64)))
                        shape = tuple(matrix.shape)
                        del want
                else:
                    rows[name][0].append(device_s)
                    rows[name][1].append(wall_s)
                del starts, matrix
                torch.cuda.empty_cache()
        med = {name: (statistics.median(d), statistics.median(w)) for name, (d, w) in rows.items()}
        spread = max(rows["old"][1]) - min(rows["old"][1])
        ok = same and med["new"][1] <= med["old"][1] + spread
        failed = failed or not ok
        print(f"K={K}: matrix {shape}, results {'equal' if same else 'DIFFER'}")
        for name in ("old", "new"):
            d, w = rows[name]
            print(f"   {name} route: median {med[name][0] * 1e3:9.2f} ms (HIP events) {med[name][1] * 1e3:9.2f} ms (host clock); "
                  f"min {min(w) * 1e3:9.2f}  max {max(w) * 1e3:9.2f}  ({len(w)} repetitions)")
        print(f"   old / new = {med['old'][1] / med['new'][1]:.1f}x by the host clock; the old route's spread is {spread * 1e3:.2f} ms: "
              f"{'not slower' if ok else 'SLOWER'}")
        # the fill kernel alone: K full rows, one segment
        m = shape[1]
        counts = torch.randint(0, 40, (K * m,), device=dev, dtype=torch.int32).to(torch.float32)
        words = rt.track_matrix_shape()["row_words"]
        table = np.zeros(K * words + 2, dtype=np.int64)
        body = table[: K * words].reshape(K, words)
        body[:, 0], body[:, 1], body[:, 2], body[:, 3], body[:, 4] = np.arange(K) * m, m, 0, 0, m - 1
        body[:, 5] = np.full(K, 1.25, dtype=np.float64).view(np.int64)
        table_t = torch.from_numpy(table).to(dev)
        out = torch.empty((K, m), dtype=torch.float64, device=dev)
        stream = _dp._stream_ptr(out)

        def fill():
            rc = lib.rocco_hip_track_matrix_fill(solver.handle, counts.data_ptr(), K * m, table_t.data_ptr(), K, table_t[K * words:].data_ptr(), 1, m,
                                                 0, float(STEP), 1.0, 5, 0, out.data_ptr(), stream)
            assert rc == 0, rc

        times = [timed(torch, fill)[1] for _ in range(args.reps + 1)][1:]
        t = statistics.median(times)
        check = torch.round(counts[:1000].to(torch.float64) * 1.25, decimals=5)
        assert torch.equal(out[0, :1000], check)
        print(f"   fill kernel alone: {K} x {m} float64, median {t * 1e3:.3f} ms of {len(times)}; {K * m * 12 / 1e9:.2f} GB (4 B read + 8 B written "
              f"per element) = {K * m * 12 / t / 1e12:.2f} TB/s")
        del records, counts, out, table_t
        torch.cuda.empty_cache()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
