"""What the reference's own code returned on the seeded inputs of the tests that compare the oracle against it, kept
as SHA-256 digests of the exact bytes (and, for the objective, as a number: see objective_rounding) in
tests/golden/reference_digests.json, written by tests/golden/make_golden_reference_digests.py where the reference is
built, so that those tests need nothing outside the repository."""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")


def digest(*values) -> str:
    """Digest of the dtype, shape and bytes of every value in turn (a dict: of its keys and values, keys sorted)."""
    h = hashlib.sha256()
    for v in values:
        parts = [x for k in sorted(v) for x in (k, v[k])] if isinstance(v, dict) else [v]
        for p in parts:
            a = np.ascontiguousarray(np.asarray(p))
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def objective_rounding(scores, costs, solution) -> float:
    """How far two summation orders of the objective -(scores @ solution) + costs @ |diff(solution)| can put it apart
    (n eps times the magnitudes summed, twice).  NumPy hands both dots to BLAS, whose order follows the CPU and the
    thread count, so the reference's own objective differs from host to host in its last bits: a recorded objective is
    compared within this bound, everything else bit for bit."""
    sol = np.asarray(solution, dtype=np.float64)
    magnitude = float(np.abs(np.asarray(scores, dtype=np.float64)) @ sol)
    if sol.size > 1:
        magnitude += float(np.abs(np.asarray(costs, dtype=np.float64)) @ np.abs(np.diff(sol)))
    return 2.0 * sol.size * np.finfo(np.float64).eps * magnitude


def recorded(group: str) -> dict:
    """case name -> the reference's recorded output (a digest, or an objective), for one group of cases."""
    with open(PATH) as fh:
        return json.load(fh)[group]
