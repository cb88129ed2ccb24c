#!/usr/bin/env python3
"""Writes every case of tests/bgzf_expected.py (valid files, corrupt files, both mutation sets, the launch-turn period) as a `.case` file for
tests/tools/bgzf_inflate_san.cpp, the stand-alone sanitizer run of rocco_amd/csrc/inflate_core.h:

    python tests/tools/bgzf_inflate_cases.py DIR

A case file: int64 n_comp, n_blocks, n_out; the compressed bytes; the block table; the expected status code per block."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bgzf_expected as gx  # noqa: E402


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    files = [raw for _, raw in gx.valid_files()] + [raw for _, raw, _, _ in gx.corrupt_files()] + [gx.mutation_file(), gx.mutation_file_long(), gx.turn_period()[0]]
    for k, raw in enumerate(files):
        table = gx.table_of(raw)
        want = np.asarray([code for code, _ in gx.outcomes(raw)], dtype=np.uint8)
        with open(os.path.join(out_dir, f"{k:04d}.case"), "wb") as handle:
            handle.write(np.asarray([len(raw), table.shape[0], int(table[:, 2].sum())], dtype=np.int64).tobytes())
            handle.write(raw + table.tobytes() + want.tobytes())
    print(f"{len(files)} case files in {out_dir}")


if __name__ == "__main__":
    main()
