#!/usr/bin/env python3
"""What the REFERENCE makes of bigWig files (note (31)).

    python tests/golden/make_golden_bigwig_scores.py

Runs on the CPU.  The files of tests/bigwig_score_cases.py are written with the writer of tests/bigwig_files.py and read with
its second reader (`expected_intervals`: struct, zlib.decompress and loops; no code of the package).  That interval list is
what a stand-in ``pyBigWig`` (`assemble_golden.FakeBigWig`; values as Python floats of the float32s, as pyBigWig returns
them) hands to the reference's own ``get_bigwig_chrom_scores`` (rocco/readtracks.py:94-186) and ``generate_chrom_matrix``
(rocco/readtracks.py:521-633, ``num_processors=1``: its readers run in process).  Stored per call: what it returned, or the
exception's type and text, and the WARNING records it logged, with the directory of the files written as ``{dir}``; per file
the digest of the second reader's arrays, so that a test knows it wrote the same file again.

Writes tests/golden/bigwig_scores.npz + bigwig_scores.json (data only, no reference source)."""
import importlib
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bigwig_files as bf  # noqa: E402
import bigwig_score_cases as sc  # noqa: E402
from assemble_golden import FakeBigWig  # noqa: E402

pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco"), os.path.join(ROOT, "oracle", "_ref")]
sys.modules["rocco"] = pkg
rt = importlib.import_module("rocco.readtracks")

directory = tempfile.mkdtemp()
paths = sc.write_files(directory)
specs = sc.files()


def fake_open(path):
    """pyBigWig.open: None for what is no bigWig file, else chroms() / intervals() from the second reader."""
    name = os.path.basename(path)
    if name not in specs:
        return None
    chroms = specs[name][0]
    intervals = {}
    for chrom, _ in chroms:
        listed = bf.expected_intervals(path, chrom)
        intervals[chrom] = [(int(s), int(e), float(v)) for s, e, v in listed] or None  # (pyBigWig: None where there is none)
    return FakeBigWig({chrom: length for chrom, length in chroms}, intervals)


fake = types.ModuleType("pyBigWig")
fake.open = fake_open
rt.pyBigWig = fake


class Held(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage().replace(directory, "{dir}")])


held = Held()
rt.logger.addHandler(held)
arrays, meta = {}, {"files": {}, "scores": [], "matrix": []}
for name, (chroms, _, _) in specs.items():
    meta["files"][name] = sc.digest(paths[name], chroms)


def run(record, key, call):
    held.records = []
    try:
        intervals, values = call()
    except (OSError, ValueError, RuntimeError) as exc:
        record["error"] = {"type": type(exc).__name__, "text": str(exc).replace(directory, "{dir}")}
    else:
        if intervals is None:
            assert values is None
            record["none"] = True
        else:
            arrays[f"{key}_intervals"], arrays[f"{key}_values"] = np.asarray(intervals), np.asarray(values)
            record["intervals_dtype"], record["values_dtype"] = str(np.asarray(intervals).dtype), str(np.asarray(values).dtype)
    record["log"] = held.records
    return record


for index, (name, file, chromosome, sizes, kwargs) in enumerate(sc.score_cases()):
    meta["scores"].append(run({"name": name}, f"s{index}", lambda: rt.get_bigwig_chrom_scores(
        sc.path_of(paths, directory, file), chromosome, sc.path_of(paths, directory, sizes), **kwargs)))
for index, (name, files, chromosome, kwargs) in enumerate(sc.matrix_cases()):
    meta["matrix"].append(run({"name": name}, f"m{index}", lambda: rt.generate_chrom_matrix(
        chromosome, [sc.path_of(paths, directory, f) for f in files], paths[sc.SIZES_FILE], 50, num_processors=1, **kwargs)))

np.savez_compressed(os.path.join(HERE, "bigwig_scores.npz"), **arrays)
with open(os.path.join(HERE, "bigwig_scores.json"), "w", encoding="utf-8") as handle:
    json.dump(meta, handle, indent=1, sort_keys=True)
print(f"wrote {len(meta['scores'])} get_bigwig_chrom_scores calls, {len(meta['matrix'])} generate_chrom_matrix calls, {len(arrays)} arrays")
for kind in ("scores", "matrix"):
    for r in meta[kind]:
        print(f"  {kind:7s} {r['name']:55s} ->", (r["error"]["type"] + ": " + r["error"]["text"][:70]) if "error" in r else
              ("(None, None)" if r.get("none") else "arrays"), f"[{len(r['log'])} warnings]")
