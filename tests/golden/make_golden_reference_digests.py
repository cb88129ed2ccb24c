#!/usr/bin/env python3
"""Digests of what the reference's own code returns on the seeded inputs of the tests that compare the oracle against
it (tests/reference_record.py), computed where the reference is built:

    make -C oracle ref          # oracle/_ref: libwls_ref.so, libbaseline_ref.so, the _chain_dp extension
    python tests/golden/make_golden_reference_digests.py

Writes tests/golden/reference_digests.json.  Only digests of data are written -- no reference source.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS, os.path.join(ROOT, "oracle")]

import ref_loader  # noqa: E402
import reference_record  # noqa: E402
import test_baseline_oracle  # noqa: E402
import test_oracle_golden  # noqa: E402
import test_wls_oracle  # noqa: E402

dp = ctypes.POINTER(ctypes.c_double)
out = {}

wls = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libwls_ref.so")).rocco_score_centered_wls_f64
wls.argtypes = [dp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                ctypes.c_int, ctypes.c_double, dp, dp, dp, dp, dp, dp, dp, ctypes.POINTER(ctypes.c_int)]
wls.restype = ctypes.c_int
out["wls_backend"] = {}
for name, m in test_wls_oracle.reference_backend_cases():
    K, n = m.shape
    tracks = [np.empty(n) for _ in range(6)]
    df, win = ctypes.c_double(), ctypes.c_int()
    assert wls(m.ctypes.data_as(dp), K, n, 1.0, 5.0, 0.0, 0, 31, 0.01,
               *[t.ctypes.data_as(dp) for t in tracks], ctypes.byref(df), ctypes.byref(win)) == 0
    out["wls_backend"][name] = reference_record.digest(*tracks, float(df.value), int(win.value))

baseline = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libbaseline_ref.so")).rocco_crossfit_whittaker_baseline_matrix_f64
baseline.argtypes = [dp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, dp]
baseline.restype = ctypes.c_int
out["baseline_backend"] = {}
for name, m, lam in test_baseline_oracle.reference_backend_cases():
    want = np.empty_like(m)
    assert baseline(m.ctypes.data_as(dp), m.shape[0], m.shape[1], lam, want.ctypes.data_as(dp)) == 0
    out["baseline_backend"][name] = reference_record.digest(want)

ref_dp = ref_loader.load_reference_dp()
out["chain_dp"], out["chain_dp_objective"] = {}, {}
for name, fn, call_args, kwargs in test_oracle_golden.reference_dp_cases():
    got = getattr(ref_dp, fn)(*call_args, **kwargs)
    if fn == "solve_chrom_exact":  # the objective (a BLAS dot) is kept as a number: its last bits are the host's
        out["chain_dp_objective"][name] = float(got[1])
        got = (got[0], got[2])
    out["chain_dp"][name] = reference_record.digest(*got)

with open(reference_record.PATH, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", reference_record.PATH, {k: len(v) for k, v in out.items()})
