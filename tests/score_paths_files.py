"""Test support for row f12 (scoring over BAM paths): the fixtures of tests/golden/score_paths.npz / .json -- what the
reference wrote (tests/golden/make_golden_score_paths.py) -- as files in a directory, and log records in the form the
generator stored them (level, message with the directory written as ``{dir}``).  Nothing here reads rocco_amd."""
import json
import logging
import os

import numpy as np

import bam_index_files as bif

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ["p1", "p2", "p3"]
OLD = ["header_only", "unplaced_only", "wide"]
_golden = None


def golden():
    """(arrays, meta), loaded once and left unchanged."""
    global _golden
    if _golden is None:
        with open(os.path.join(HERE, "golden", "score_paths.json"), encoding="utf-8") as handle:
            meta = json.load(handle)
        _golden = (dict(np.load(os.path.join(HERE, "golden", "score_paths.npz"))), meta)
    return _golden


def contig_names(key):
    meta = golden()[1]
    return [n for n, _ in (meta["contigs"] if key in FILES else bif.golden()[1]["files"][key]["contigs"])]


def fetch_rows(key):
    """The records of a file in the order ``fetch()`` yields them: [n, 8] = tid pos end isize flag mapq mate_same qlen."""
    arrays = golden()[0]
    table = arrays[f"rec_{key}"]
    return table[np.concatenate([arrays[f"itr_{key}_{t}"] for t in range(len(contig_names(key)))]).astype(np.int64)]


def write_files(root, with_index=True):
    """p1 .. p3 (and the three older files) with their indexes, the sizes, peaks and summit-offset files: {name: path}."""
    arrays, meta = golden()
    root = str(root)
    paths = {"dir": root}
    for key in FILES:
        paths[key] = os.path.join(root, key + ".bam")
        with open(paths[key], "wb") as handle:
            handle.write(arrays[f"bam_{key}"].tobytes())
        if with_index:
            with open(paths[key] + ".bai", "wb") as handle:
                handle.write(arrays[f"bai_{key}"].tobytes())
    for key in OLD:
        paths[key] = bif.write_indexed(root, key)
    for name, text in (("g.sizes", meta["sizes_text"]), ("peaks.bed", meta["peaks_text"]), ("summits.tsv", meta["summit_offsets_text"]),
                       ("wide.sizes", meta["skip_absent"]["sizes_text"]), ("wide.bed", meta["skip_absent"]["peaks_text"])):
        paths[name] = os.path.join(root, name)
        with open(paths[name], "w", encoding="utf-8") as handle:
            handle.write(text)
    return paths


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def logged(call, root, loggers=("rocco_amd.scores", "rocco_amd.rocco")):
    """(what ``call`` returns, its INFO and WARNING records as the generator stored the reference's)."""
    keep, held = Keep(), []
    for name in loggers:
        logger = logging.getLogger(name)
        held.append((logger, logger.level))
        logger.addHandler(keep)
        logger.setLevel(logging.INFO)
    try:
        result = call()
    finally:
        for logger, level in held:
            logger.removeHandler(keep)
            logger.setLevel(level)
    return result, [[level, message.replace(str(root), "{dir}")] for level, message in keep.records if level in ("INFO", "WARNING")]
