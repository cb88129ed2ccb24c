#!/usr/bin/env python3
"""Expected outputs of the REFERENCE's post-hoc peak-scoring helpers (rocco/scores.py) on this repository's own inputs:

    python tests/golden/make_golden_scores.py

`_peak_signal_stat` per peak, `EmpiricalNull.survival` per length bin, `_assign_length_bins`, and
scipy.stats.false_discovery_control (what score_peaks calls at rocco/scores.py:583) -- the parts of `score_peaks` that do
not touch a BAM file (the function itself cannot run here: it counts reads with pysam).  `rocco.scores` is imported
with a dummy `pysam` module in place.  Writes tests/golden/scores_vectors.npz (the defaults: percentile 75, pc 1, row
scale 1000) and tests/golden/scores_offdefault_vectors.npz (`_peak_signal_stat` over percentiles, pseudocounts, row
scales and non-finite counts on part of the cases of tests/peak_scores_expected.py; `EmpiricalNull.survival` for NaN,
infinite and tied statistics) -- data only.  A file whose arrays come out as they are recorded is left as it is (an
archive written again differs in its time stamps)."""
import importlib
import os
import sys
import types

import warnings

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco"), os.path.join(ROOT, "oracle", "_ref")]
sys.modules["rocco"] = pkg
dummy = types.ModuleType("pysam")
dummy.AlignedSegment = type("AlignedSegment", (), {})
sys.modules.setdefault("pysam", dummy)
scores = importlib.import_module("rocco.scores")
sys.path.insert(0, os.path.dirname(HERE))
import peak_scores_expected as cases  # noqa: E402


def write(name, arrays):
    path = os.path.join(HERE, name)
    if os.path.exists(path):
        with np.load(path) as old:
            if sorted(old.files) == sorted(arrays) and all(
                    old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v, equal_nan=old[k].dtype.kind == "f")
                    for k, v in arrays.items()):
                print(f"{path}: unchanged, left as it is")
                return
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")


rng = np.random.default_rng(31)
out = {}
for name, P, K in (("small", 40, 3), ("wide", 2500, 12), ("many", 20000, 5), ("one_sample", 300, 1)):
    lengths = rng.integers(50, 4000, size=P).astype(np.float64)
    counts = rng.gamma(2.0, 30.0, size=(P, K)) * (lengths[:, None] / 500.0)
    counts[rng.random((P, K)) < 0.05] = 0.0
    binned, reps = scores._assign_length_bins(lengths, max_bins=24)
    nulls = {int(r): rng.gamma(2.0, 1.2, size=int(rng.integers(20, 500))) for r in reps}
    sig = np.array([scores._peak_signal_stat(counts[i], lengths[i], row_scale=1000, pc=1) for i in range(P)])
    pvals = np.array([scores.EmpiricalNull(nulls[int(binned[i])]).survival(sig[i]) for i in range(P)])
    qvals = stats.false_discovery_control(pvals, method="bh")
    out[f"{name}_counts"], out[f"{name}_lengths"], out[f"{name}_binned"] = counts, lengths, binned
    out[f"{name}_null_keys"] = np.array(sorted(nulls))
    for k, v in nulls.items():
        out[f"{name}_null_{k}"] = v
    out[f"{name}_sig"], out[f"{name}_pvals"], out[f"{name}_qvals"] = sig, pvals, qvals
out["names"] = np.array(["small", "wide", "many", "one_sample"])
write("scores_vectors.npz", out)

# ---- off the defaults --------------------------------------------------------------------------------------------------
out = {}
all_cases = cases.shape_cases()
with warnings.catch_warnings(), np.errstate(all="ignore"):
    warnings.simplefilter("ignore", RuntimeWarning)  # log2(0), inf - inf: what these inputs are for
    for index in cases.FIXTURE_CASES:
        case = all_cases[index]
        assert case["K"] <= 33 and case["P"] <= 257
        counts, lengths = cases.inputs(case)
        counts, lengths = counts[:cases.FIXTURE_ROWS], lengths[:cases.FIXTURE_ROWS]
        out[f"case{index}_counts"], out[f"case{index}_lengths"] = counts, lengths
        for j, (pc, row_scale) in enumerate(cases.parameters(case)):
            out[f"case{index}_sig{j}"] = np.array(
                [[scores._peak_signal_stat(counts[i], lengths[i], row_scale=row_scale, pc=pc, percentile=percentile)
                  for i in range(counts.shape[0])] for percentile in cases.PERCENTILES])
            out[f"case{index}_params{j}"] = np.array([pc, row_scale])
    for name, null, stat in cases.survival_cases():
        model = scores.EmpiricalNull(null)
        out[f"survival_{name}_null"], out[f"survival_{name}_stat"] = null, stat
        out[f"survival_{name}_vector"] = model.survival(stat)
        out[f"survival_{name}_scalars"] = np.array([model.survival(float(x)) for x in stat])
out["case_indexes"] = np.array(cases.FIXTURE_CASES)
out["percentiles"] = np.array(cases.PERCENTILES, dtype=np.float64)
out["survival_names"] = np.array([name for name, _, _ in cases.survival_cases()])
write("scores_offdefault_vectors.npz", out)
