#!/usr/bin/env python3
"""Expected outputs of the REFERENCE's score_dispersion_chrom (rocco/rocco.py:307-355):

    python tests/golden/make_golden_dispersion.py

`rocco.rocco` is imported under an empty package object with a dummy `pysam`, as make_golden_composed.py does (the
package import fails on the absent pysam; no pysam code is on any path used here).

Recorded in tests/golden/dispersion_vectors.npz -- data only, no reference source:
  * matrices `matrix_<id>`: K in {2, 3, 8, 9, 33, 100, 101, 137} x 48 columns in float64 and float32, values rounded to
    two decimals (many ties); column 0 constant, column 1 holds a NaN, columns 2-5 hold +inf, -inf, both, and +inf in
    more than half of the rows; one K x 1 matrix per K; one 1 x 48 matrix;
  * cases `case_<i>`: JSON {matrix, method, rng, power} and `expected_<i>`, what the reference returned: `mad`, `std` and
    `iqr` over several `rng` (one reversed), `power` 1 and 2, every method name at K = 1 (an unknown one included);
  * errors `error_<i>`: JSON {matrix or shape, kwargs, class, text}: a percentile out of range, an unknown method, a 1-D
    input, and `tstd` at K != n -- the reference's own failure, on file because rocco_amd computes the per-column
    trimmed standard deviation there instead (see score_dispersion_chrom's docstring)."""
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")

pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco"), os.path.join(ROOT, "oracle", "_ref")]
sys.modules["rocco"] = pkg
dummy = types.ModuleType("pysam")
dummy.AlignedSegment = type("AlignedSegment", (), {})
sys.modules.setdefault("pysam", dummy)
impl = importlib.import_module("rocco.rocco")

KS = (2, 3, 8, 9, 33, 100, 101, 137)
N = 48
RNGS = ((25, 75), (10, 90), (12.5, 87.5), (0, 100), (33, 66.6), (75, 25), (50, 50), (1, 99))


def tied_matrix(K, n, rng):
    m = np.round(rng.gamma(2.0, 1.5, size=(K, n)), 2)
    if n >= 6:
        inf = np.inf
        m[:, 0] = 1.25
        m[int(rng.integers(0, K)), 1] = np.nan
        m[int(rng.integers(0, K)), 2] = inf
        m[int(rng.integers(0, K)), 3] = -inf
        m[0, 4], m[K - 1, 4] = inf, -inf
        m[: K // 2 + 1, 5] = inf
    return m


out, cases, errors = {}, [], []


def record(matrix_id, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # inf - inf inside np.std / np.percentile
        got = impl.score_dispersion_chrom(out[f"matrix_{matrix_id}"], **kwargs)
    assert got.dtype == np.float64
    out[f"expected_{len(cases)}"] = got
    cases.append(json.dumps(dict(matrix=matrix_id, **kwargs)))


def record_error(matrix, matrix_id, **kwargs):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            impl.score_dispersion_chrom(matrix, **kwargs)
    except Exception as exc:  # the class and the text are the record
        entry = dict(kwargs=kwargs, **{"class": type(exc).__name__, "text": str(exc)})
        entry.update(matrix=matrix_id) if matrix_id is not None else entry.update(shape=list(np.shape(matrix)))
        errors.append(json.dumps(entry))
        print(f"  error {type(exc).__name__}: {exc}")
        return
    raise AssertionError(f"the reference accepted {kwargs}")


gen = np.random.default_rng(307355)
for K in KS:
    m = tied_matrix(K, N, gen)
    out[f"matrix_k{K}_f64"] = m
    out[f"matrix_k{K}_f32"] = m.astype(np.float32)
    out[f"matrix_k{K}_n1"] = tied_matrix(K, 1, gen)
    for idx, tag in enumerate(("f64", "f32")):
        name = f"k{K}_{tag}"
        record(name, method="mad")
        record(name, method="std")
        record(name, method="mad", power=2)
        record(name, method="std", power=2)
        for r in (RNGS if idx == 0 else RNGS[:1] + RNGS[4:6]):
            record(name, method="iqr", rng=list(r))
        record(name, method="iqr", rng=[10, 90], power=2)
    for method in ("mad", "std", "iqr"):
        record(f"k{K}_n1", method=method)
# spellings the reference normalises
record("k9_f64", method=" M-A_D ")
record("k9_f64", method="IQR", rng=[20, 80])
# K = 1: zeros to the power, before the method is looked at
out["matrix_k1"] = tied_matrix(1, N, gen)
for method in ("mad", "iqr", "std", "tstd", "no such method"):
    record("k1", method=method)
record("k1", method="mad", power=2)
record("k1", method="std", power=0)

record_error(out["matrix_k9_f64"], "k9_f64", method="iqr", rng=[25, 101])
record_error(out["matrix_k9_f64"], "k9_f64", method="iqr", rng=[-1, 75])
record_error(out["matrix_k9_f64"], "k9_f64", method="variance")
record_error(np.arange(5.0), None, method="mad")
record_error(out["matrix_k9_f64"], "k9_f64", method="tstd")  # K = 9, n = 48: the reference's own call cannot run

out["cases"] = np.array(cases)
out["errors"] = np.array(errors)
path = os.path.join(HERE, "dispersion_vectors.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {len(cases)} cases, {len(errors)} errors, {os.path.getsize(path) / 1e3:.0f} kB")
