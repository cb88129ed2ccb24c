#!/usr/bin/env python3
"""Times row f5 (decoded alignment records -> binned coverage, rocco_amd/csrc/count.hip) at the size of a chr1 track.

    python tests/tools/alignment_count_bench.py --build-only      (anywhere hipcc is: the stand-alone builds of count.hip)
    python tests/tools/alignment_count_bench.py [--records 20000000] [--tracks 1 8] [--reps 10]     (on the MI355X)
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/alignment_count_bench.py --reps 3 --tracks 1

One synthetic track: N position-sorted records over 248 Mb, step 50 (4.96 M bins), either spread evenly ("uniform") or
half of them in 20 000 peaks of 500 bp ("peaky"); a batch is 8 such tracks in one call.  The builds are timed in turn,
alternating, each call from the host's clock to the call's own closing synchronise (the records are in HBM before, the
counts are in HBM after): the library's entry point, and count.hip built alone with and without its LDS window
(-DROCCO_COUNT_NO_LDS_AGGREGATION: every +1 / -1 is a global atomic) and with a counting launch of up to 2 048 and
8 192 workgroups instead of the library's 512 (-DROCCO_COUNT_TOOL_MAX_GRID).  All must agree bit for bit.

The floor the rate is held against: 16 B read per record; per bin 4 B zeroed, 4 B read by the tile sums, 4 B read by the
scan and 4 B of float32 written (16 B per bin)."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
BUILD = os.path.join(HERE, "build")
VARIANTS = {"lds_window": [], "global_atomics_only": ["-DROCCO_COUNT_NO_LDS_AGGREGATION"],
            "lds_window_grid_2048": ["-DROCCO_COUNT_TOOL_MAX_GRID=2048"], "lds_window_grid_8192": ["-DROCCO_COUNT_TOOL_MAX_GRID=8192"]}
SPAN, STEP = 248_000_000, 50


def lib_path(name):
    return os.path.join(BUILD, f"libcount_{name}.so")


def build():
    os.makedirs(BUILD, exist_ok=True)
    for name, flags in VARIANTS.items():
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                        "-DROCCO_COUNT_STANDALONE", *flags, os.path.join(ROOT, "rocco_amd", "csrc", "count.hip"), "-o", lib_path(name)],
                       check=True)


def synthetic_track(torch, n, kind, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    pos = torch.randint(0, SPAN - 1000, (n,), generator=g, device=device, dtype=torch.int64)
    if kind == "peaky":
        centres = torch.randint(0, SPAN - 1000, (20000,), generator=g, device=device, dtype=torch.int64)
        pick = torch.randint(0, 20000, (n // 2,), generator=g, device=device)
        pos[: n // 2] = (centres[pick] + torch.randint(0, 500, (n // 2,), generator=g, device=device)).clamp_(0, SPAN - 1000)
    pos = torch.sort(pos).values.to(torch.int32)
    end = pos + 50
    flag = (torch.randint(0, 2, (n,), generator=g, device=device, dtype=torch.int32) * 16).to(torch.int16)
    mapq = torch.randint(0, 61, (n,), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
    return pos, end, torch.zeros(n, dtype=torch.int32, device=device), flag, mapq, torch.ones(n, dtype=torch.uint8, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kinds", nargs="+", default=["uniform", "peaky"])
    args = ap.parse_args()
    if args.build_only:
        build()
        return
    import torch

    from rocco_amd import _native
    from rocco_amd import dp as _dp
    from rocco_amd.readtracks import CountOptions, CountRegion

    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda:0")
    lib = _native.load()
    solver = _native.solver_for(0)
    alone = {}
    for name in VARIANTS:
        if not os.path.isfile(lib_path(name)):
            raise SystemExit(f"{lib_path(name)} missing: run with --build-only first")
        alone[name] = ctypes.CDLL(lib_path(name))
        alone[name].rocco_count_standalone_scratch_bytes.restype = ctypes.c_size_t
        alone[name].rocco_count_standalone.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 7
    bins = (SPAN - 1) // STEP + 1
    print(f"device {torch.cuda.get_device_name(0)}; {args.records} records per track, {bins} bins per track, step {STEP}")
    for kind in args.kinds:
        for K in args.tracks:
            tracks = [synthetic_track(torch, args.records, kind, 100 + k, dev) for k in range(K)]
            cat = [torch.cat([t[i] for t in tracks]) for i in range(6)]
            del tracks
            opts, regs = (CountOptions * K)(), (CountRegion * K)()
            rec_off, out_off, maxima = (ctypes.c_longlong * (K + 1))(), (ctypes.c_longlong * K)(), (ctypes.c_longlong * K)()
            for k in range(K):
                opts[k] = CountOptions(flag_exclude=3844, min_mapq=10, read_length=50, max_insert_size=1000, min_template_length=-1)
                regs[k] = CountRegion(0, SPAN, STEP, bins)
                rec_off[k + 1], out_off[k] = (k + 1) * args.records, k * bins
            nbytes = alone["lds_window"].rocco_count_standalone_scratch_bytes(rec_off, K, opts, regs, out_off)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            outs = {name: torch.empty(K * bins, dtype=torch.float32, device=dev) for name in ["library", *VARIANTS]}
            stream = _dp._stream_ptr(scratch)
            ptrs = [c.data_ptr() for c in cat]

            def run(name):
                if name == "library":
                    rc = lib.rocco_hip_count_alignment_records_batch(solver.handle, *ptrs, rec_off, K, ctypes.cast(opts, ctypes.c_void_p),
                                                                     ctypes.cast(regs, ctypes.c_void_p), out_off, 0, outs[name].data_ptr(),
                                                                     maxima, stream)
                else:
                    rc = alone[name].rocco_count_standalone(*ptrs, ctypes.cast(rec_off, ctypes.c_void_p), K, ctypes.cast(opts, ctypes.c_void_p),
                                                            ctypes.cast(regs, ctypes.c_void_p), ctypes.cast(out_off, ctypes.c_void_p),
                                                            outs[name].data_ptr(), ctypes.cast(maxima, ctypes.c_void_p), scratch.data_ptr(), stream)
                assert rc == 0, (name, rc)

            times = {name: [] for name in outs}
            for rep in range(args.reps + 2):  # two warm-up rounds
                for name in outs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(name)  # (ends in its own stream synchronise)
                    if rep >= 2:
                        times[name].append(time.perf_counter() - t0)
            for name in VARIANTS:
                assert torch.equal(outs[name], outs["library"]), f"{name} differs from the library"
            floor = K * (16 * args.records + 16 * bins)
            kept = int((outs["library"] > 0).sum())
            print(f"{kind:8s} K={K}: deepest bin {int(outs['library'].max())}, {kept} bins covered, largest magnitude {max(maxima)}, "
                  f"floor {floor / 1e6:.0f} MB")
            for name, ts in times.items():
                med = statistics.median(ts)
                print(f"    {name:20s} median {med * 1e3:8.3f} ms  min {min(ts) * 1e3:8.3f}  max {max(ts) * 1e3:8.3f}  ({len(ts)} calls)  "
                      f"{floor / med / 1e9:7.1f} GB/s of the floor's bytes")
            del cat, outs, scratch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
