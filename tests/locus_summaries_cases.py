"""What the locus-summary tests share: the fixture of tests/golden/make_golden_locus_summaries.py, read once, and a NumPy
stand-in for the device calls behind rocco_amd.inference's `_DeviceVector` (the contract of include/rocco_hip.h restated
in NumPy), so that the host logic around the kernels runs where there is no GPU."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_QUANTILES = [0.0, 0.01, 0.05, 0.25, 0.50, 0.75, 0.95, 0.975, 0.99, 1.0]


@functools.lru_cache(maxsize=None)
def golden():
    data = np.load(os.path.join(HERE, "golden", "locus_summaries_vectors.npz"))
    return {key: data[key] for key in data.files}


def cases(name):
    return [json.loads(str(entry)) for entry in golden()[name]]


def errors(function):
    return [entry for entry in cases("errors") if entry["function"] == function]


def same_bits(a, b) -> bool:
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def same_float(a, b) -> bool:
    """bit equality, any NaN equal to any NaN"""
    return (np.isnan(a) and np.isnan(b)) or same_bits(a, b)


def key_sorted(values):
    """ascending in the select's key order: -inf .. finite (-0.0 before +0.0) .. +inf .. NaN"""
    v = np.asarray(values, dtype=np.float64)
    bits = v.view(np.uint64)
    keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
    keys = np.where(np.isnan(v), np.uint64(0xFFFFFFFFFFFFFFFF), keys)
    return v[np.argsort(keys, kind="stable")]


class NumpyVector:
    def __init__(self, values):
        self.x = np.asarray(values, dtype=np.float64)
        self.n = int(self.x.shape[0])

    def counts(self):
        x = self.x
        return int(np.isnan(x).sum()), int((x == -np.inf).sum()), int((x == np.inf).sum()), int((x <= 0.0).sum())

    def select(self, ranks, mode=0, center=0.0):
        with np.errstate(all="ignore"):
            v = self.x if mode == 0 else np.where(np.isfinite(self.x), np.abs(self.x - center), np.nan)
        ordered = key_sorted(v)
        return [float(ordered[r]) for r in ranks]

    def last_passing(self, fdr):
        """as rocco_hip_sort_f64 + rocco_hip_bh_last_passing_rank_f64: the sort orders bit patterns (sign-set NaNs first,
        the others last), the kernel steps over the leading NaNs"""
        bits = self.x.view(np.uint64)
        ordered = self.x[np.argsort(np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63)), kind="stable")]
        lead = int((np.isnan(ordered) & np.signbit(ordered)).sum())
        assert not np.isnan(ordered[lead:self.n - int(np.isnan(ordered[lead:]).sum())]).any()
        m = self.n
        passing = np.nonzero(ordered[lead:] <= float(fdr) * (np.arange(1, m - lead + 1) / float(m)))[0]
        i = lead + int(passing.max()) if passing.size else -1
        return i, float(ordered[max(i, 0)])

    def at_most(self, cutoff):
        return self.x <= cutoff

    def divide_finite(self, divisor):
        out = np.zeros_like(self.x)
        finite = np.isfinite(self.x)
        out[finite] = self.x[finite] / divisor
        return out

    def threshold_mask(self, divisor, threshold, floor_value, use_floor):
        mask = self.divide_finite(divisor) > threshold
        return mask & (self.x > floor_value) if use_floor else mask
