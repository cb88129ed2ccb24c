#!/usr/bin/env python3
"""Times the BGZF inflate on the device (rocco_amd/csrc/bgzf_inflate.hip: DEFLATE and CRC32 in HIP, one wavefront per block)
beside the host's (`rocco_amd.bam.inflate_bgzf`: Python's zlib on a thread pool), in one run on the same machine.

    timeout 900 python tests/tools/bgzf_inflate_bench.py [--records 4000000] [--reps 5] > profiles/bgzf_inflate_bench.txt

Input: the record stream of tests/tools/bam_decode_bench.py (a block of 4 096 synthetic records repeated until `records`
records), cut into 65 280-byte BGZF blocks and compressed by Python's zlib at levels 1, 6 and 0.  Per level, as GB/s of
INFLATED bytes, the median of `reps` repetitions after one warm-up:
  device, in HBM    `rocco_hip_bgzf_inflate` with the compressed bytes and the block table already in HBM (HIP events around the
                    call, which ends in its own stream synchronise)
  device + upload   the same with the upload of table and compressed bytes from pinned memory inside the timed window
  device, file      `inflate_bgzf_device` over the file's bytes, wall clock: the block headers walked in Python, the pinned
                    buffer allocated and filled, upload, inflate
  host              `inflate_bgzf` over the same bytes with its default thread pool, wall clock
The device's output is compared with the host's byte for byte before anything is timed.  No speed bar: the comparison point
is the host figure of the same run."""
import argparse
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]

from bam_decode_bench import record_block  # noqa: E402


def bgzf(data, level, threads):
    def one(at):
        chunk = bytes(data[at: at + 0xFF00])
        packer = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = packer.compress(chunk) + packer.flush()
        return (struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, 25 + len(cdata)) + cdata +
                struct.pack("<II", zlib.crc32(chunk), len(chunk)))

    with ThreadPoolExecutor(max_workers=threads) as pool:
        return b"".join(pool.map(one, range(0, len(data), 0xFF00)))


def timed_events(torch, call, reps):
    times = []
    for rep in range(reps + 1):  # one warm-up
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        call()
        done.record()
        done.synchronize()
        if rep >= 1:
            times.append(begin.elapsed_time(done) / 1e3)
    return times


def timed_wall(torch, call, reps):
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep >= 1:
            times.append(time.perf_counter() - begin)
    return times


def line(label, times, n_bytes, n_blocks):
    med = statistics.median(times)
    return (f"  {label:<16} median {med * 1e3:9.2f} ms (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}) = {n_bytes / med / 1e9:7.2f} GB/s of "
            f"inflated bytes, {n_blocks / med / 1e3:8.1f} k blocks/s")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--records", type=int, default=4_000_000)
    parser.add_argument("--reps", type=int, default=5)
    args = parser.parse_args()
    import torch

    from rocco_amd import bam

    if not torch.cuda.is_available():
        raise SystemExit("bgzf_inflate_bench: no HIP device (there is no CPU fallback and nothing to time without one)")
    dev = torch.device("cuda:0")
    block = record_block(4096, 7)
    stream = np.tile(np.frombuffer(block, dtype=np.uint8), max(args.records // 4096, 1))
    n_bytes, threads = int(stream.size), bam._default_threads()
    print(f"device {torch.cuda.get_device_name(0)}; {stream.size // len(block) * 4096} records, {n_bytes} inflated bytes in 65 280-byte BGZF "
          f"blocks; host: {threads} threads, zlib {zlib.ZLIB_RUNTIME_VERSION}; {args.reps} repetitions after one warm-up, medians")
    for level in (1, 6, 0):
        packed = bgzf(stream, level, threads)
        raw = memoryview(packed)
        blocks = bam._bgzf_blocks(raw, "<bench>")
        base, end = blocks[0][1], blocks[-1][2]
        table = bam.bgzf_block_table(blocks, base)
        head = table.size * 8
        staged = bam._host_buffer(head + end - base)
        staged[:head] = table.reshape(-1).view(np.uint8)
        staged[head:] = np.frombuffer(raw[base:end], dtype=np.uint8)
        pinned = torch.from_numpy(staged)
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        up = pinned.to(dev)

        def inflate(up=up):
            _, report = bam.inflate_blocks_device(up[head:], up[:head].view(torch.int64), out)
            assert report["block"] == -1, report

        inflate()
        want = bam.inflate_bgzf(packed)
        assert out.cpu().numpy().tobytes() == want.tobytes(), "the device's bytes differ from the host's"
        del want
        print(f"level {level}: {len(blocks)} blocks, {len(packed)} compressed bytes ({len(packed) / n_bytes:.3f} of the inflated), pinned: {pinned.is_pinned()}")
        print(line("device, in HBM", timed_events(torch, inflate, args.reps), n_bytes, len(blocks)))
        print(line("device + upload", timed_events(torch, lambda: inflate(pinned.to(dev, non_blocking=True)), args.reps), n_bytes, len(blocks)))
        print(line("device, file", timed_wall(torch, lambda: bam.inflate_bgzf_device(packed, device=dev), args.reps), n_bytes, len(blocks)))
        print(line("host", timed_wall(torch, lambda: bam.inflate_bgzf(packed), args.reps), n_bytes, len(blocks)), flush=True)
        del up, out, pinned, staged


if __name__ == "__main__":
    main()
