#!/usr/bin/env python3
"""Expected outputs of the REFERENCE's score-track budget estimate where the lag cap passes 1023 lags, and its verdicts on
tracks with non-finite values:

    make -C oracle ref
    python tests/golden/make_golden_budget_long_lag.py

rocco.inference.estimate_budget_nonnull_fraction_from_score_track (+ details), _estimate_effective_sample_size and
rocco.rocco._resolve_chrom_gamma, imported as tests/golden/make_golden_budget.py imports them.  The inputs are built by
tests/budget_stats_cases.py (ramp tracks whose autocorrelation stays positive for thousands of lags; the 4000-long
"signal" track with one value replaced).  Every stored long-lag case is checked here, and again from the stored numbers
by tests/test_budget_stats_cases_host.py: the truncation lag lies where the case wants it, and every pair sum of
Geyer's rule up to and including the terminating one is farther than 1e-6 from zero -- what makes "the truncation lag
must be equal" a fair demand on sums that are not the reference's FFT.  Writes tests/golden/budget_long_lag_vectors.npz
-- data only, no reference source."""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import budget_stats_cases as bc  # noqa: E402

pkg = types.ModuleType("rocco")
pkg.__path__ = [os.path.join(REFERENCE, "rocco"), os.path.join(ROOT, "oracle", "_ref")]
sys.modules["rocco"] = pkg
dummy = types.ModuleType("pysam")
dummy.AlignedSegment = type("AlignedSegment", (), {})
sys.modules.setdefault("pysam", dummy)
inference = importlib.import_module("rocco.inference")
impl = importlib.import_module("rocco.rocco")

out = {}


def plain(details):
    return {k: (v if isinstance(v, (str, bool)) else float(v)) for k, v in details.items()}


def gamma_row(gamma, meta):
    return [gamma, meta["autocorrelation_time"], meta["characteristic_run_length"], meta["positive_score_median"],
            meta["positive_score_count"], meta["gamma_raw"]]


def checked_pairs(label, values, max_lag, lags_used, wanted_above):
    """Pair sums (direct lagged products) up to the terminating one; fails unless the case is what it is stored for."""
    pairs, used, _tau = bc.geyer_pairs(values, max_lag)
    assert used == lags_used, (label, used, lags_used)
    assert lags_used > wanted_above, (label, lags_used, wanted_above)
    assert pairs.size > 0 and float(np.min(np.abs(pairs))) > bc.PAIR_MARGIN, (label, float(np.min(np.abs(pairs))))
    return pairs


# ---- C: ramps whose truncation lag passes one, two and four lag chunks of the kernel ----
ess_names, est_names = [], []
for n in bc.RAMP_LENGTHS:
    s = bc.ramp_track(n)
    out[f"ramp_n{n}_scores"] = s
    _frac, base = inference.estimate_budget_nonnull_fraction_from_score_track(s, dependence_lag_hint=256, num_null_draws=6,
                                                                              return_details=True)
    soft = bc.soft_counts(s, base["null_center"], base["null_scale"])
    for max_lag in bc.ess_max_lags(n):
        ess, tau, used = inference._estimate_effective_sample_size(soft, max_lag)
        name = f"ramp_n{n}_ess{max_lag}"
        wanted = bc.wanted_lags_above(n, max_lag)
        pairs = checked_pairs(name, soft, max_lag, used, wanted)
        _p, _u, direct_tau = bc.geyer_pairs(soft, max_lag)
        assert abs(direct_tau - tau) <= 1e-12 * tau, (name, direct_tau, tau)
        ess_names.append(name)
        out[f"{name}_result"] = np.array([ess, tau, used], dtype=np.float64)
        out[f"{name}_check"] = np.array([wanted, float(np.min(np.abs(pairs))), float(pairs[-1])], dtype=np.float64)
        print(f"{name}: lags_used {used}  tau {tau:.6f}  min |pair| {np.min(np.abs(pairs)):.3e}  direct/fft-1 {direct_tau / tau - 1:.1e}")
    for hint in bc.ESTIMATE_HINTS:
        frac, det = inference.estimate_budget_nonnull_fraction_from_score_track(s, dependence_lag_hint=hint, num_null_draws=6,
                                                                                return_details=True)
        name = f"ramp_n{n}_h{hint}"
        soft_h = bc.soft_counts(s, det["null_center"], det["null_scale"])
        wanted = bc.wanted_lags_above(n, int(det["ess_max_lag"]))
        pairs = checked_pairs(name, soft_h, int(det["ess_max_lag"]), int(det["ess_lags_used"]), wanted)
        gamma, meta = impl._resolve_chrom_gamma("chrT", {"gamma": None}, s, det)
        est_names.append(name)
        out[f"{name}_fraction"] = np.array([frac])
        out[f"{name}_details"] = np.array([json.dumps(plain(det))])
        out[f"{name}_gamma"] = np.array(gamma_row(gamma, meta), dtype=np.float64)
        out[f"{name}_check"] = np.array([wanted, float(np.min(np.abs(pairs))), float(pairs[-1])], dtype=np.float64)
        print(f"{name}: ess_max_lag {int(det['ess_max_lag'])}  lags_used {int(det['ess_lags_used'])}  tau {det['autocorrelation_time']:.6f}")
out["ess_names"] = np.array(ess_names)
out["estimate_names"] = np.array(est_names)


# ---- E: what the reference does with non-finite values (the tracks themselves are rebuilt by budget_stats_cases) ----
def verdict(call):
    try:
        with np.errstate(all="ignore"):
            got = call()
    except Exception as exc:  # noqa: BLE001 (the verdict IS the exception)
        return {"raises": type(exc).__name__, "message": str(exc)}
    return {"returns": got}


verdicts = {}
for name, s in bc.nonfinite_tracks():
    def estimate(s=s):
        frac, det = inference.estimate_budget_nonnull_fraction_from_score_track(s, num_null_draws=6, return_details=True)
        return {"fraction": float(frac), "details": plain(det)}

    def ess(s=s):
        return [float(v) for v in inference._estimate_effective_sample_size(s, bc.NONFINITE_ESS_MAX_LAG)]

    def gamma(s=s):
        g, meta = impl._resolve_chrom_gamma("chrT", {"gamma": None}, s, {"autocorrelation_time": 3.25})
        return [float(v) for v in gamma_row(g, meta)]

    verdicts[name] = {"estimate": verdict(estimate), "ess": verdict(ess), "gamma": verdict(gamma)}
    e = verdicts[name]["estimate"]
    print(f"{name}: estimate {'raises ' + e['raises'] if 'raises' in e else 'returns %.6g' % e['returns']['fraction']}"
          f"  ess {verdicts[name]['ess']}  gamma {verdicts[name]['gamma'].get('returns', verdicts[name]['gamma'])}")
out["nonfinite_verdicts"] = np.array([json.dumps(verdicts)])

path = os.path.join(HERE, "budget_long_lag_vectors.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {len(ess_names)} ESS cases, {len(est_names)} estimates, {len(verdicts)} non-finite tracks, "
      f"{os.path.getsize(path) / 1e6:.2f} MB")
