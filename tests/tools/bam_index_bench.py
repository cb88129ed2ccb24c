#!/usr/bin/env python3
"""Times row f11 (contigs of BAM files read through the .bai index, rocco_amd/bam.py: read_alignment_spans) against the
whole-file decode of the same file in the same run.

    python tests/tools/bam_index_bench.py [--records 20000000] [--reps 5] > profiles/bam_index_bench.txt

Input: the synthetic record stream of tests/tools/bam_decode_bench.py (blocks of 4 096 records of 160 to 200 bytes), dealt in
equal shares to 25 contigs, behind a BAM header, compressed by Python's zlib at level 1 into 65 280-byte BGZF blocks; its
index is written with tests/bam_index_files.py (pseudo-bins and one bin per contig, from the known record offsets).
  one contig    read_alignment_spans([(file, contig)]) against read_alignment_file(file), in both inflate modes
  K = 8 files   eight hard links of the file: one call of eight (file, contig) pairs against eight calls of one pair
Timed with HIP events around the entry points (each ends synchronised), one warm-up + `reps` repetitions, the median.
Nothing is asserted about speed: the expectation is that the cost falls roughly with the contig's share of the file."""
import argparse
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bam_decode_bench as dec  # noqa: E402
import bam_index_files as bif  # noqa: E402

N_REF = dec.N_REF
BLOCK = 0xFF00


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--records", type=int, default=20_000_000)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--contig", type=int, default=7)
    args = parser.parse_args()
    import torch

    from rocco_amd import bam

    block = np.frombuffer(dec.record_block(4096, 7), dtype=np.uint8)
    starts, at = [], 0
    while at < block.size:
        starts.append(at)
        at += 4 + struct.unpack_from("<i", block, at)[0]
    starts = np.asarray(starts)
    per_contig = max(args.records // N_REF // 4096, 1)  # blocks of 4 096 records per contig
    header = b"BAM\1" + struct.pack("<ii", 0, N_REF) + b"".join(
        struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", 1 << 30) for name in (b"chr%d" % k for k in range(N_REF)))
    parts = [np.frombuffer(header, dtype=np.uint8)]
    for tid in range(N_REF):
        mine = block.copy()
        mine[starts + 4] = tid  # (refID, little-endian: its other three bytes are 0)
        parts.append(np.tile(mine, per_contig))
    stream = np.concatenate(parts)
    records, share = per_contig * 4096 * N_REF, per_contig * block.size
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    # the compressed size of every block gives its file offset; a contig's inflated bounds give its virtual offsets
    chunks = [dec.bgzf(stream[at: at + (BLOCK << 8)], threads) for at in range(0, stream.size, BLOCK << 8)]
    raw = b"".join(chunks) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    table = bif.block_table(raw)
    refs = []
    for tid in range(N_REF):
        begin, end = len(header) + tid * share, len(header) + (tid + 1) * share
        v = (bif.voffset(table, len(raw), begin), bif.voffset(table, len(raw), end))
        refs.append({"bins": {0: [v]}, "linear": [v[0]], "pseudo": v + (per_contig * 4096, 0)})
    print(f"device {torch.cuda.get_device_name(0)}; {records} records on {N_REF} contigs, {stream.size} inflated bytes, {len(raw)} compressed, "
          f"{len(table)} BGZF blocks; a contig holds {share} inflated bytes ({100.0 / N_REF:.1f} % of the file); {args.reps} repetitions "
          "after one warm-up, HIP events, medians")
    contig = f"chr{args.contig}"
    with tempfile.TemporaryDirectory() as folder:
        paths = [os.path.join(folder, f"bench{k}.bam") for k in range(8)]
        with open(paths[0], "wb") as handle:
            handle.write(raw)
        with open(paths[0] + ".bai", "wb") as handle:
            handle.write(bif.bai_bytes(refs, 0))
        for path in paths[1:]:
            os.link(paths[0], path)
            os.link(paths[0] + ".bai", path + ".bai")
        del raw, chunks, stream, parts
        for mode in ("host", "device"):
            med_w, low_w, high_w, (file, _) = dec.timed(torch, lambda: bam.read_alignment_file(paths[0], inflate=mode), args.reps)
            want = file.records[contig]
            med_c, low_c, high_c, got = dec.timed(torch, lambda: bam.read_alignment_spans([(paths[0], contig)], inflate=mode), args.reps)
            assert len(got[0]) == per_contig * 4096 and all(torch.equal(getattr(got[0], f), getattr(want, f)) for f in ("pos", "end", "flag", "qlen"))
            del file, want
            print(f"inflate={mode}: whole file {med_w:.1f} ms (min {low_w:.1f}, max {high_w:.1f}); one contig through the index "
                  f"{med_c:.1f} ms (min {low_c:.1f}, max {high_c:.1f}) = {100.0 * med_c / med_w:.1f} % of the whole-file decode")
            med_k, low_k, high_k, got = dec.timed(torch, lambda: bam.read_alignment_spans([(p, contig) for p in paths], inflate=mode), args.reps)
            med_1, low_1, high_1, _ = dec.timed(torch, lambda: [bam.read_alignment_spans([(p, contig)], inflate=mode) for p in paths], args.reps)
            assert len(got) == 8 and all(len(g) == per_contig * 4096 for g in got)
            print(f"inflate={mode}: K = 8 files of one contig in one call {med_k:.1f} ms (min {low_k:.1f}, max {high_k:.1f}); eight single "
                  f"calls {med_1:.1f} ms (min {low_1:.1f}, max {high_1:.1f})")


if __name__ == "__main__":
    main()
