#!/usr/bin/env python3
"""Times the barcode census on a synthetic fragments file (DESIGN.md note (35)): the whole call with the inflate on the host
and on the device, its stages on the first slab (line pass, insert + settle into a fresh table, the records and the order on
the host), and the rate against ``collections.Counter`` over the same inflated text on the host, in the same run.

    python tests/tools/barcode_census_bench.py [--lines 10000000] [--barcodes 100000] [--repeat 3] [--out profiles/barcode_census_bench.txt]

Two files: barcodes drawn under a skewed distribution (the cube of a uniform draw picks the barcode: the most frequent tenth
of the barcodes has about 46 % of the lines), and one dominant barcode (90 % of the lines meet at one counter, that is at one
L2 atomic unit).  The files are written here: fixed-width lines built with NumPy, BGZF blocks through zlib on a thread pool,
a ``.tbi`` with one bin and the pseudo-bin (what `rocco_amd.tabix_index` needs of an index; no htslib).  Host clock with a
device synchronisation on either side, medians of ``--repeat`` calls after a warm-up.  No bar is set: the figures are
written down."""
import argparse
import collections
import concurrent.futures
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def bgzf_block(data: bytes, level: int = 1) -> bytes:
    deflate = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = deflate.compress(data) + deflate.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def write_fragments(path: str, name: str, text: bytes) -> None:
    view = memoryview(text)
    with concurrent.futures.ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as pool:
        blocks = list(pool.map(lambda lo: bgzf_block(bytes(view[lo: lo + 0xFF00])), range(0, len(text), 0xFF00)))
    with open(path, "wb") as out:
        for block in blocks:
            out.write(block)
        out.write(bgzf_block(b""))
    end = sum(len(b) for b in blocks) << 16
    names = name.encode() + b"\x00"
    index = b"TBI\x01" + struct.pack("<8i", 1, 0x10000, 1, 2, 3, ord("#"), 0, len(names)) + names
    index += struct.pack("<i", 2) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", 0, end)
    index += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", 0, end, 0, 0) + struct.pack("<i", 0)
    with open(path + ".tbi", "wb") as out:
        out.write(bgzf_block(index) + bgzf_block(b""))


def digits(values: np.ndarray, width: int) -> np.ndarray:
    out = np.empty((values.shape[0], width), dtype=np.uint8)
    for k in range(width):
        out[:, width - 1 - k] = 48 + (values // 10 ** k) % 10
    return out


def synthetic(n_lines: int, codes: np.ndarray) -> bytes:
    """``chr1<TAB>start(9)<TAB>end(9)<TAB>BC<code(8)>-1<TAB>1`` per line, sorted by start."""
    rng = np.random.default_rng(5)
    starts = np.cumsum(rng.integers(0, 40, size=n_lines))
    row = np.frombuffer(b"chr1\t000000000\t000000000\tBC00000000-1\t1\n", dtype=np.uint8)
    lines = np.tile(row, (n_lines, 1))
    lines[:, 5:14], lines[:, 15:24], lines[:, 27:35] = digits(starts, 9), digits(starts + 200, 9), digits(codes, 8)
    return lines.tobytes()


def median_ms(call, repeat: int) -> float:
    import torch

    call()
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main() -> None:
    import torch

    from rocco_amd import fragments as fr
    from rocco_amd.bam import inflate_bgzf

    parser = argparse.ArgumentParser()
    parser.add_argument("--lines", type=int, default=10000000)
    parser.add_argument("--barcodes", type=int, default=100000)
    parser.add_argument("--repeat", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "barcode_census_bench.txt"))
    opts = parser.parse_args()
    said = []

    def say(text):
        print(text, flush=True)
        said.append(text)

    work = tempfile.mkdtemp(prefix="barcode_census_bench_")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    draws = {"skewed": np.minimum((opts.barcodes * rng.random(opts.lines) ** 3).astype(np.int64), opts.barcodes - 1),
             "dominant": np.where(rng.random(opts.lines) < 0.9, 0, rng.integers(0, opts.barcodes, size=opts.lines))}
    say(f"barcode_census_bench: {opts.lines} lines, {opts.barcodes} barcodes, device {torch.cuda.get_device_name(0)}, "
        f"medians of {opts.repeat} calls after a warm-up")
    for name, codes in draws.items():
        text = synthetic(opts.lines, codes)
        path = os.path.join(work, name + ".tsv.gz")
        write_fragments(path, "chr1", text)
        top = int(np.bincount(codes).max())
        say(f"{name}: {len(text)} bytes of text, {os.path.getsize(path)} bytes compressed, the most frequent barcode has {top} lines "
            f"({100.0 * top / opts.lines:.1f} %)")
        results = {}
        for inflate in ("host", "device"):
            results[inflate] = fr.barcode_census(path, device=dev, inflate=inflate)
            ms = median_ms(lambda: fr.barcode_census(path, device=dev, inflate=inflate), opts.repeat)
            say(f"  whole call, inflate={inflate:6s} {ms:10.2f} ms  {opts.lines / ms / 1e3:8.2f} M lines/s   {results[inflate].stats}")
        assert results["host"].barcodes == results["device"].barcodes and np.array_equal(results["host"].records, results["device"].records)
        # the stages on the first slab of the default size
        slab = torch.from_numpy(np.frombuffer(text[: text.rfind(b"\n", 0, fr.DEFAULT_SLAB_BYTES) + 1], dtype=np.uint8).copy()).to(dev)
        starts, report = fr.lines_device(slab)
        say(f"  first slab: {int(slab.shape[0])} bytes, {report['lines']} lines")
        say(f"    stage lines                    {median_ms(lambda: fr.lines_device(slab), opts.repeat):10.2f} ms")

        def insert():
            table = fr.BarcodeCensusTable(dev)
            table.insert(slab, starts)
            return table

        say(f"    stage table + insert + settle  {median_ms(insert, opts.repeat):10.2f} ms")
        table = insert()
        say(f"    stage rehash to twice the slots{median_ms(lambda: rehash(fr, table), opts.repeat):10.2f} ms")
        say(f"    stage records + order on host  {median_ms(table.census, opts.repeat):10.2f} ms   ({table.entries} entries)")
        # the host: collections.Counter over the same inflated text, in the same run
        t0 = time.perf_counter()
        inflated = bytes(inflate_bgzf(path))
        t1 = time.perf_counter()
        counted = collections.Counter(line.split(b"\t", 4)[3] for line in inflated.split(b"\n") if line)
        t2 = time.perf_counter()
        got = results["device"]
        assert len(counted) == len(got) and all(counted[b] == n for b, n in zip(got.barcodes, got.records.tolist()))
        device_ms = median_ms(lambda: fr.barcode_census(path, device=dev, inflate="device"), 1)
        say(f"  host: inflate {1e3 * (t1 - t0):10.2f} ms, collections.Counter over the text {1e3 * (t2 - t1):10.2f} ms "
            f"({opts.lines / (t2 - t1) / 1e6:.2f} M lines/s); the census equals it ({len(counted)} barcodes)")
        say(f"  rate: whole call with the device inflate {device_ms:.2f} ms = {1e3 * (t2 - t0) / device_ms:.1f} x the host's inflate + Counter, "
            f"{1e3 * (t2 - t1) / device_ms:.1f} x the Counter alone")
        del slab, starts, table, inflated, counted, text
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w", encoding="utf-8") as handle:
        handle.write("\n".join(said) + "\n")


def rehash(fr, table):
    """One rehash of the table's entries into twice the slots (the table itself is left as it is)."""
    import torch

    from rocco_amd import _native, dp

    slots = torch.empty(2 * table.capacity, dtype=torch.int64, device=table.device)
    counts = torch.empty(2 * table.capacity, dtype=torch.int64, device=table.device)
    _native.check(_native.load().rocco_hip_barcode_census_rehash(
        _native.solver_for(table.device.index).handle, table.slots.data_ptr(), table.counts.data_ptr(), table.capacity, slots.data_ptr(),
        counts.data_ptr(), 2 * table.capacity, table.arena_hashes.data_ptr(), table.entries, table.mask, dp._stream_ptr(slots)), "rehash")


if __name__ == "__main__":
    main()
