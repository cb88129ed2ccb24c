#!/usr/bin/env python3
"""Times row f10 end to end (a bigWig path -> the dense track of a chromosome in HBM: container on the host, upload, inflate, section
decode, dense fill; rocco_amd/bigwig.py over csrc/bgzf_inflate.hip and csrc/bigwig_sections.hip) at the size of chr1, for one file and for
a batch of 8, against the host twin of the decode over `inflate="host"` in the same run.

    python tests/tools/bigwig_read_bench.py [--bins 4979128] [--files 1 8] [--reps 3] > profiles/bigwig_read_bench.txt

Input: fixedStep tracks at 50 bp over chr1 (248 956 422 bp: 4 979 128 items in sections of 1 024, zlib level 6), written by the writer
of tests/bigwig_files.py from a seed.
Device route, stage by stage on the host clock (every stage ends with the device idle): the container (`open_bigwig` and the block
table, cache cleared), upload + inflate (`inflate_chrom_blocks`, "device"), the decode (`decode_sections_device`: both calls), the dense
fill per file (`bigwig_dense_fill_device`).  Host route: `inflate_chrom_blocks` with "host" (zlib on the thread pool, one upload), the
slots copied back, `decode_sections_host` (one thread), the intervals uploaded, the same dense fill.  One warm-up of each, then `reps`
repetitions; medians.  The two routes' intervals are compared bit for bit once per batch size.
The floor of the decode is stated as the bytes of the sections read once + 24 B written per interval, and what the decode makes of it.
No speed bar: nothing is compared against pyBigWig, which is not installed where this runs.  Exits 1 if the routes differ."""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CHR1, STEP, PER_SECTION = 248_956_422, 50, 1024


def write_track(bf, np, path, bins, seed):
    rng = np.random.default_rng(seed)
    values = np.round(rng.gamma(1.0, 2.0, size=bins), 3).astype(np.float32)
    sections = [bf.section(0, 3, values[lo: lo + PER_SECTION], start=STEP * lo, step=STEP, span=STEP) for lo in range(0, bins, PER_SECTION)]
    bf.write_bigwig(path, [("chr1", CHR1)], sections)
    return len(sections)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=CHR1 // STEP)
    ap.add_argument("--files", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch

    import bigwig_files as bf
    from rocco_amd import bigwig
    from rocco_amd import readtracks as rt

    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda:0")
    print(f"device {torch.cuda.get_device_name(0)}; chr1 = {CHR1} bp, {args.bins} fixedStep items at {STEP} bp in sections of {PER_SECTION}; "
          f"shape {bigwig.sections_shape()}")

    def clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    failed = False
    with tempfile.TemporaryDirectory() as directory:
        paths = [os.path.join(directory, f"track{k}.bw") for k in range(max(args.files))]
        for k, path in enumerate(paths):
            n_sections = write_track(bf, np, path, args.bins, 500 + k)
        print(f"{len(paths)} files of {os.path.getsize(paths[0]) / 1e6:.1f} MB, {n_sections} data blocks each")
        for K in args.files:
            stages = {"device": {}, "host": {}}

            def route(mode, keep):
                def note(stage, seconds):
                    if keep:
                        stages[mode].setdefault(stage, []).append(seconds)

                bigwig.clear_bigwig_cache()
                wanted, t = clock(lambda: [(bigwig.open_bigwig(p), "chr1") for p in paths[:K]])
                layout_s = clock(lambda: [bigwig.chrom_blocks(f, c) for f, c in wanted])[1]
                note("container", t + layout_s)
                (slots, table, produced, first), t = clock(lambda: bigwig.inflate_chrom_blocks(wanted, dev, mode))
                note("upload + inflate", t)
                ids, lengths = [f.chroms[c][0] for f, c in wanted], [f.chroms[c][1] for f, c in wanted]
                if mode == "device":
                    got, t = clock(lambda: bigwig.decode_sections_device(slots, table.reshape(-1), produced, first, ids, lengths))
                    note("decode", t)
                else:
                    host, t = clock(lambda: (slots.cpu().numpy(), table.cpu().numpy(), produced.cpu().numpy()))
                    note("slots back to the host", t)
                    got, t = clock(lambda: bigwig.decode_sections_host(*host, first, ids, lengths))
                    note("decode", t)
                    _, t = clock(lambda: got.update({k: torch.from_numpy(got[k]).to(dev) for k in ("starts", "ends", "values")}))
                    note("intervals to the device", t)
                offsets = got["file_offsets"]
                fills, t = clock(lambda: [rt.bigwig_dense_fill_device(*(got[k][int(offsets[j]): int(offsets[j + 1])] for k in ("starts", "ends", "values")),
                                                                      device=dev) for j in range(K)])
                note("dense fill", t)
                return got, int(slots.numel()), int(produced.sum()), fills

            results = {}
            for rep in range(args.reps + 1):  # one warm-up
                for mode in ("host", "device"):
                    got, slot_bytes, section_bytes, fills = route(mode, rep > 0)
                    if rep == 0:
                        results[mode] = [got[k].cpu().numpy().view(np.uint64) for k in ("starts", "ends", "values")] + \
                            [f[2].cpu().numpy().view(np.uint64) for f in fills]
                    del got, fills
                    torch.cuda.empty_cache()
            same = all(np.array_equal(a, b) for a, b in zip(results["device"], results["host"]))
            failed = failed or not same
            intervals = int(results["device"][0].size)
            floor = section_bytes + 24 * intervals
            print(f"K={K}: {intervals} intervals from {section_bytes / 1e6:.1f} MB of sections; the two routes' intervals and tracks "
                  f"{'are equal' if same else 'DIFFER'}")
            for mode in ("device", "host"):
                total = 0.0
                for stage, times in stages[mode].items():
                    med = statistics.median(times)
                    total += med
                    print(f"   {mode:6s} route  {stage:24s} median {med * 1e3:9.2f} ms  (min {min(times) * 1e3:9.2f}, max {max(times) * 1e3:9.2f}, {len(times)} repetitions)")
                print(f"   {mode:6s} route  {'all stages':24s}        {total * 1e3:9.2f} ms")
            decode = statistics.median(stages["device"]["decode"])
            print(f"   decode floor: {section_bytes / 1e6:.1f} MB of sections read once + 24 B x {intervals} intervals written = {floor / 1e6:.1f} MB; "
                  f"the device decode (two calls: facts, scan, emit, two waits) makes {floor / decode / 1e9:.1f} GB/s of it; "
                  f"host twin / device decode = {statistics.median(stages['host']['decode']) / decode:.0f}x")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
