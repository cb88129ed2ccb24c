#!/usr/bin/env python3
"""Times the fragments path on a synthetic file (DESIGN.md note (34)): inflate, lines, fields and count of one contig, with the
inflate on the device against the same path with ``inflate="host"``.

    python tests/tools/fragments_bench.py [--lines 2000000] [--repeat 5] > profiles/fragments_bench.txt

The file is written here: BGZF blocks through zlib, and a ``.tbi`` with one bin and the pseudo-bin per contig (what
`rocco_amd.tabix_index` needs of an index; no htslib).  Host clock with a device synchronisation on either side, medians of
``--repeat`` calls after a warm-up.  No bar is set: nobody has measured this path before."""
import argparse
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def bgzf_block(data: bytes) -> bytes:
    deflate = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = deflate.compress(data) + deflate.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def write_fragments(path: str, contigs) -> None:
    """``contigs``: [(name, text)].  Every contig begins a block; blocks of 0xff00 bytes."""
    spans, at = [], 0
    with open(path, "wb") as out:
        for name, text in contigs:
            begin = at << 16
            for lo in range(0, len(text), 0xFF00):
                block = bgzf_block(text[lo: lo + 0xFF00])
                out.write(block)
                at += len(block)
            spans.append((name, begin, at << 16))
        out.write(bgzf_block(b""))
    names = b"".join(name.encode() + b"\x00" for name, _, _ in spans)
    index = b"TBI\x01" + struct.pack("<8i", len(spans), 0x10000, 1, 2, 3, ord("#"), 0, len(names)) + names
    for _, begin, end in spans:
        index += struct.pack("<i", 2) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", begin, end)
        index += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", begin, end, 0, 0) + struct.pack("<i", 0)
    with open(path + ".tbi", "wb") as out:
        for lo in range(0, len(index), 0xFF00):
            out.write(bgzf_block(index[lo: lo + 0xFF00]))
        out.write(bgzf_block(b""))


def synthetic(n_lines: int, seed: int, contig: str) -> bytes:
    rng = np.random.default_rng(seed)
    starts = np.cumsum(rng.integers(0, 60, size=n_lines))
    ends = starts + rng.integers(30, 800, size=n_lines)
    codes = rng.integers(0, 5000, size=n_lines)
    counts = rng.integers(1, 5, size=n_lines)
    return "".join(f"{contig}\t{s}\t{e}\tBC{c:012d}-1\t{w}\n" for s, e, c, w in zip(starts, ends, codes, counts)).encode()


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

    parser = argparse.ArgumentParser()
    parser.add_argument("--lines", type=int, default=2000000)
    parser.add_argument("--repeat", type=int, default=5)
    opts = parser.parse_args()
    work = tempfile.mkdtemp(prefix="fragments_bench_")
    path = os.path.join(work, "f.tsv.gz")
    text = synthetic(opts.lines, 1, "chr1")
    write_fragments(path, [("chr1", text)])
    allow = os.path.join(work, "allow.txt")
    with open(allow, "w") as handle:
        handle.write("".join(f"BC{c:012d}-1\n" for c in range(0, 5000, 3)))
    dev = torch.device("cuda:0")
    top = int(text.rsplit(b"\n", 2)[-2].split(b"\t")[2]) + 1
    print(f"fragments_bench: {opts.lines} lines, {len(text)} bytes of text, {os.path.getsize(path)} bytes compressed, "
          f"allow-list of {len(range(0, 5000, 3))} barcodes, device {torch.cuda.get_device_name(0)}")
    sources = [fr.FragmentsSource(path), fr.FragmentsSource(path, allow)]
    results = {}
    for inflate in ("device", "host"):
        def whole():
            fr.clear_fragments_cache()
            return fr.count_fragments_regions([(s, "chr1", 0, top, 50, "coverage", 0) for s in sources], device=dev, inflate=inflate)

        results[inflate] = [c.cpu().numpy() for c in whole()]
        print(f"  inflate={inflate:6s}: file -> counts of 2 sources (1 inflate, 1 line pass, 2 field passes, 1 count) {median_ms(whole, opts.repeat):9.2f} ms")
    assert all(np.array_equal(a, b) for a, b in zip(results["device"], results["host"]))
    fr.clear_fragments_cache()
    stream = fr._stream_of(sources[0], "chr1", {})
    for inflate in ("device", "host"):
        call = (lambda: fr._bam._group_bytes_device([stream], dev)) if inflate == "device" else (lambda: fr._bam._group_bytes_host([stream], dev, None))
        print(f"  stage inflate ({inflate:6s}) {median_ms(call, opts.repeat):9.2f} ms")
    data = fr._bam._group_bytes_device([stream], dev)
    print(f"  stage lines            {median_ms(lambda: fr.lines_device(data), opts.repeat):9.2f} ms")
    starts, report = fr.lines_device(data)
    for name, packed in (("no list", fr._NO_LIST), ("list", sources[1].allowlist())):
        call = lambda: fr.fields_device(data, starts, False, [0, report["lines"]], [0], ["chr1"], [packed])  # noqa: E731
        print(f"  stage fields ({name:7s}) {median_ms(call, opts.repeat):9.2f} ms")
    lines, _ = fr.fields_device(data, starts, False, [0, report["lines"]], [0], ["chr1"], [fr._NO_LIST])
    for mode in ("coverage", "cutsite", "center"):
        call = lambda: fr.count_lines_batch_device([lines], [(0, top, 50)], [mode], [0])  # noqa: E731
        print(f"  stage count ({mode:8s}) {median_ms(call, opts.repeat):9.2f} ms")
    print(f"  lines {report['lines']}, bins {((top - 1) // 50) + 1}; results of the two inflate modes equal")


if __name__ == "__main__":
    main()
