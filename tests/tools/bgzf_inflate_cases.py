#!/usr/bin/env python3
"""Writes every case of tests/bgzf_expected.py (valid files, corrupt files, both mutation sets, the launch-turn period) as BGZF-framed
`.case` files, and the three stream lists of tests/bigwig_files.py (valid, corrupt, mutated) as zlib-framed ones, for
tests/tools/bgzf_inflate_san.cpp, the stand-alone sanitizer run of rocco_amd/csrc/inflate_core.h:

    python tests/tools/bgzf_inflate_cases.py DIR

A case file: int64 framing (0 BGZF, 1 zlib), n_comp, n_blocks, n_out; the compressed bytes; the block table; the expected status code per
block."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bgzf_expected as gx  # noqa: E402
import bigwig_files as bf  # noqa: E402


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    cases = []  # (framing, compressed bytes, table, n_out, expected codes)
    files = [raw for _, raw in gx.valid_files()] + [raw for _, raw, _, _ in gx.corrupt_files()] + [gx.mutation_file(), gx.mutation_file_long(), gx.turn_period()[0]]
    for raw in files:
        table = gx.table_of(raw)
        cases.append((0, raw, table, int(table[:, 2].sum()), [code for code, _ in gx.outcomes(raw)]))
    lists = ([s[1:] for s in bf.valid_streams()], [s[1:4] for s in bf.corrupt_streams()], [(span, capacity, 0) for span, capacity in bf.mutated_streams()])
    for streams in lists:
        comp, table, n_out = bf.table_of(streams, guard=0)  # (no guard bytes: the output buffer ends where the last slot ends)
        cases.append((1, comp, table, n_out, [bf.expected_status(*s)[0] & 0xFF for s in streams]))
    for k, (framing, comp, table, n_out, want) in enumerate(cases):
        with open(os.path.join(out_dir, f"{k:04d}.case"), "wb") as handle:
            handle.write(np.asarray([framing, len(comp), table.shape[0], n_out], dtype=np.int64).tobytes())
            handle.write(comp + table.tobytes() + np.asarray(want, dtype=np.uint8).tobytes())
    print(f"{len(cases)} case files in {out_dir} ({len(files)} BGZF-framed, {len(lists)} zlib-framed)")


if __name__ == "__main__":
    main()
