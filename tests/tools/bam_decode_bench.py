#!/usr/bin/env python3
"""Times row f8 (the inflated bytes of a BAM file -> record offsets -> record arrays, rocco_amd/csrc/bam_records.hip) and, apart
from it, the host's BGZF inflate (rocco_amd/bam.py).

    python tests/tools/bam_decode_bench.py [--records 20000000] [--reps 5] > profiles/bam_decode_bench.txt

Input: one inflated record stream made on the host: a block of 4 096 synthetic records (75-base reads with names of 8 to 30
bytes, one to three CIGAR operations, random sequence and quality bytes, a 12-byte tag area; 160 to 200 bytes each), repeated
until `records` records; all on contig 0 of 25.
  walk      rocco_hip_bam_walk_records at the default segment size, guess_mode 1 (and once at guess_mode 0, where the one
            repairing wavefront walks the whole stream: the cost of a stream on which every guess is wrong; over the first
            `--wrong-guess-records` records)
  fields    rocco_hip_bam_record_fields over the offsets
Timed with HIP events around each entry point (the bytes in HBM before; every entry point ends in its own stream
synchronise), one warm-up + `reps` repetitions, the median; bytes per second are the stream's bytes over that time.
  inflate   rocco_amd.bam.inflate_bgzf (wall clock, its default thread pool) over the same stream compressed by Python's
            zlib at level 1 into 65 280-byte BGZF blocks; `--inflate-records` bounds its share of the stream.
  reader    rocco_amd.bam.read_alignment_file (wall clock between two device synchronisations) over a temporary file: a BAM
            header for the 25 contigs in front of the whole stream, compressed as above; in both inflate modes, at the default
            slab size and at 32 MiB slabs (many carries and joins).  It uses public names only, so `--legs reader` times the
            package of any commit that has the reader: the bar for a change to the reader is, per line, a median no more than
            the earlier commit's median times (1 + its own (max - min) / median).
No speed bar for the kernels: the reference's htslib does not travel to the GPU machine."""
import argparse
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
N_REF = 25


def record_block(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        name = bytes(rng.integers(48, 123, size=int(rng.integers(7, 30))).astype(np.uint8)) + b"\0"
        ops = [(0, 75)] if k % 3 else [(4, 5), (0, 60), (4, 10)]
        body = name + b"".join(struct.pack("<I", (n << 4) | op) for op, n in ops) + bytes(rng.integers(0, 256, size=38 + 75 + 12).astype(np.uint8))
        out.append(struct.pack("<iiiBBHHHiiii", 32 + len(body), 0, 1000 + k, len(name), int(rng.integers(0, 61)), 4680, len(ops),
                               16 if k % 2 else 0, 75, 0 if k % 5 else -1, 1200 + k, 250) + body)
    return b"".join(out)


def bgzf(data, threads):
    def one(at):
        chunk = bytes(data[at: at + 0xFF00])
        packer = zlib.compressobj(1, zlib.DEFLATED, -15)
        cdata = packer.compress(chunk) + packer.flush()
        return (struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, 25 + len(cdata)) + cdata +
                struct.pack("<II", zlib.crc32(chunk), len(chunk)))

    with ThreadPoolExecutor(max_workers=threads) as pool:
        return b"".join(pool.map(one, range(0, len(data), 0xFF00)))


def timed(torch, call, reps):
    times, result = [], None
    for rep in range(reps + 1):  # one warm-up
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        result = call()
        done.record()
        done.synchronize()
        if rep >= 1:
            times.append(begin.elapsed_time(done))
    return statistics.median(times), min(times), max(times), result


def reader_leg(torch, bam, stream, records, threads, reps):
    header = b"BAM\1" + struct.pack("<ii", 0, N_REF) + b"".join(
        struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", 1 << 30) for name in (b"chr%d" % k for k in range(N_REF)))
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, "bench.bam")
        with open(path, "wb") as handle:
            handle.write(bgzf(np.concatenate([np.frombuffer(header, dtype=np.uint8), stream]), threads))
            handle.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        print(f"reader: {os.path.getsize(path)} compressed bytes, {len(header) + stream.size} inflated, {records} records")
        for mode in ("host", "device"):
            for slab_bytes in (None, 32 << 20):
                how = {} if slab_bytes is None else {"slab_bytes": slab_bytes}
                times = []
                for rep in range(reps + 1):  # one warm-up
                    torch.cuda.synchronize()
                    begin = time.perf_counter()
                    file, unplaced = bam.read_alignment_file(path, inflate=mode, **how)
                    torch.cuda.synchronize()
                    if rep >= 1:
                        times.append(time.perf_counter() - begin)
                    assert len(file.records["chr0"]) == records and unplaced == 0
                    del file
                med = statistics.median(times)
                print(f"reader inflate={mode} slab_bytes={'default' if slab_bytes is None else slab_bytes}: median {med * 1e3:.1f} ms "
                      f"(min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) = {stream.size / med / 1e9:.2f} GB/s of inflated bytes")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--legs", default="kernels,reader", help="of kernels (walk, fields, inflate) and reader")
    parser.add_argument("--records", type=int, default=20_000_000)
    parser.add_argument("--inflate-records", type=int, default=4_000_000)
    parser.add_argument("--wrong-guess-records", type=int, default=1_000_000)
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()
    legs = set(args.legs.split(","))
    import torch

    from rocco_amd import bam

    block = record_block(4096, 7)
    repeats = max(args.records // 4096, 1)
    stream = np.tile(np.frombuffer(block, dtype=np.uint8), repeats)
    records, n_bytes = repeats * 4096, int(stream.size)
    print(f"device {torch.cuda.get_device_name(0)}; {records} records, {n_bytes} inflated bytes ({n_bytes / records:.1f} per record), "
          f"segment {bam.DEFAULT_SEGMENT_BYTES} bytes, guess depth {bam.GUESS_DEPTH}, {args.reps} repetitions after one warm-up")
    if "reader" in legs:
        reader_leg(torch, bam, stream, records, max(1, min(16, len(os.sched_getaffinity(0)))), args.reps)
    if "kernels" not in legs:
        return
    bytes_t = torch.from_numpy(stream).to("cuda:0")
    head = bytes_t[: min(repeats, max(args.wrong_guess_records // 4096, 1)) * len(block)]
    for mode, label, data in ((1, "walk", bytes_t), (0, "walk, every guess wrong (guess_mode 0)", head)):
        med, low, high, (offsets, report) = timed(torch, lambda: bam.walk_records_device(data, 0, N_REF, guess_mode=mode),
                                                  args.reps if mode else 1)
        assert report["records"] == data.shape[0] // len(block) * 4096 and report["error"] == 0
        print(f"{label}: {report['records']} records, median {med:.2f} ms (min {low:.2f}, max {high:.2f}) = "
              f"{data.shape[0] / med / 1e6:.2f} GB/s of inflated bytes; {report['segments']} segments, {report['wrong_guesses']} wrong guesses, "
              f"{report['repair_rounds']} walked again")
    offsets, report = bam.walk_records_device(bytes_t, 0, N_REF)
    med, low, high, (_, firsts, error) = timed(torch, lambda: bam.record_fields_device(bytes_t, offsets, N_REF), args.reps)
    assert error == (0, -1) and firsts[1] == records
    print(f"fields: median {med:.2f} ms (min {low:.2f}, max {high:.2f}) = {n_bytes / med / 1e6:.2f} GB/s of inflated bytes, "
          f"{records / med / 1e3:.1f} M records/s")
    del bytes_t, offsets
    share = stream[: min(repeats, max(args.inflate_records // 4096, 1)) * len(block)]
    threads = bam._default_threads()
    packed = bgzf(share, threads)
    times = []
    for rep in range(min(args.reps, 3) + 1):
        begin = time.perf_counter()
        out = bam.inflate_bgzf(packed)
        if rep >= 1:
            times.append(time.perf_counter() - begin)
    assert out.size == share.size
    print(f"inflate (host, {threads} threads, zlib {zlib.ZLIB_RUNTIME_VERSION}): {share.size} inflated bytes from {len(packed)} compressed, "
          f"median {statistics.median(times) * 1e3:.1f} ms (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) = "
          f"{share.size / statistics.median(times) / 1e9:.2f} GB/s of inflated bytes")


if __name__ == "__main__":
    main()
