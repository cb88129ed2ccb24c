#!/usr/bin/env python3
"""Expected outputs of the REFERENCE's summaries along the locus axis: cscores_quantiles (rocco/rocco.py:358-395) and
_robust_scale, benjamini_hochberg, _standardize_wls_z_scores, candidate_mask_from_wls (rocco/inference.py:32-37, 382-443):

    python tests/golden/make_golden_locus_summaries.py

`rocco.rocco` and `rocco.inference` are imported under an empty package object with a dummy `pysam`, as
make_golden_dispersion.py does.

Recorded in tests/golden/locus_summaries_vectors.npz -- data only, no reference source:
  * `numpy_version`, and `signatures`: JSON {function: str(inspect.signature)};
  * score vectors `scores_<id>`: lengths 1, 2, 3, 10, 255-257, 8191-8193 and 49157 (three chunks of a counting pass + 5)
    of gamma values rounded to two decimals (heavy ties); 90 % exact zeros; all equal over three chunks; negative; mixed
    sign; with +inf / -inf; with one NaN; subnormals; 1 + k 2^-52 (keys that differ only in the last digit pass).  No
    vector holds -0.0 (NumPy returns whichever zero its partition left at a rank);
  * `quantile_cases`: JSON {scores, quantiles (null: the default), add_newlines, text}; `quantile_values_<i>`: what
    np.quantile(..., method="higher") gave for each quantile, in the order given;
  * z vectors `z_<id>` and `mask_cases`: JSON {z, tail_z, min_signal, null_scale}; `standardized_<id>`, `mask_<i>`;
  * `scale_cases`: JSON {values, floor, result} over `values_<id>` (_robust_scale);
  * p vectors `p_<id>` (ties at the cutoff, NaNs of both signs) and `bh_cases`: JSON {p, fdr, passing}; `bh_mask_<i>`;
  * `errors`: JSON {function, input, kwargs, class, text}."""
import importlib
import inspect
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
ref_rocco = importlib.import_module("rocco.rocco")
ref_inference = importlib.import_module("rocco.inference")

CHUNK = 16384  # values per workgroup of a counting pass (csrc/select.hip)
out = {"numpy_version": np.array(np.__version__)}
out["signatures"] = np.array(json.dumps({
    "cscores_quantiles": str(inspect.signature(ref_rocco.cscores_quantiles)),
    "_robust_scale": str(inspect.signature(ref_inference._robust_scale)),
    "benjamini_hochberg": str(inspect.signature(ref_inference.benjamini_hochberg)),
    "_standardize_wls_z_scores": str(inspect.signature(ref_inference._standardize_wls_z_scores)),
    "candidate_mask_from_wls": str(inspect.signature(ref_inference.candidate_mask_from_wls)),
}))
errors = []


def record_error(function, fn, value, input_id, **kwargs):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn(value, **kwargs)
    except Exception as exc:  # the class and the text are the record
        errors.append(json.dumps({"function": function, "input": input_id, "kwargs": kwargs, "class": type(exc).__name__,
                                  "text": str(exc)}))
        print(f"  error {function}: {type(exc).__name__}: {exc}")
        return
    raise AssertionError(f"the reference accepted {function}({input_id}, {kwargs})")


# ---- score vectors and their quantiles ---------------------------------------------------------------------------
gen = np.random.default_rng(358395)


def ties(n):
    return np.round(gen.gamma(2.0, 1.5, size=n), 2)


for n in (1, 2, 3, 10, 255, 256, 257, 8191, 8192, 8193, 3 * CHUNK + 5):
    out[f"scores_gamma{n}"] = ties(n)
zeros = ties(8193)
zeros[gen.random(8193) < 0.9] = 0.0
out["scores_zeros90"] = zeros
out["scores_equal"] = np.full(3 * CHUNK + 5, 2.75)
out["scores_negative"] = -ties(257) - 0.01
out["scores_mixed"] = np.round(gen.normal(0.0, 3.0, size=1000), 1) + 0.0  # (+ 0.0: no -0.0)
with_inf = ties(256)
with_inf[[3, 77]] = np.inf
with_inf[[5, 200, 201]] = -np.inf
out["scores_inf"] = with_inf
with_nan = ties(257)
with_nan[100] = np.nan
out["scores_nan"] = with_nan
out["scores_subnormal"] = np.concatenate((gen.integers(1, 1 << 20, size=200).astype(np.int64).view(np.float64),
                                          -gen.integers(1, 1 << 20, size=54).astype(np.int64).view(np.float64), [1.0e-300]))
out["scores_last_digit"] = gen.permutation(1.0 + np.arange(300) * 2.0 ** -52)
assert not any(np.any((v == 0.0) & np.signbit(v)) for k, v in out.items() if k.startswith("scores_"))

quantile_cases = []


def record_quantiles(scores_id, quantiles=None, add_newlines=True):
    scores = out[f"scores_{scores_id}"]
    kwargs = {} if quantiles is None else {"quantiles": quantiles}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        text = ref_rocco.cscores_quantiles(scores, add_newlines=add_newlines, **kwargs)
        qs = quantiles if quantiles is not None else [0.0, 0.01, 0.05, 0.25, 0.50, 0.75, 0.95, 0.975, 0.99, 1.0]
        values = np.array([np.quantile(scores, q=q, method="higher") for q in qs], dtype=np.float64)
    out[f"quantile_values_{len(quantile_cases)}"] = values
    quantile_cases.append(json.dumps({"scores": scores_id, "quantiles": None if quantiles is None else [float(q) for q in quantiles],
                                      "add_newlines": add_newlines, "text": text}))


for key in [k[len("scores_"):] for k in list(out) if k.startswith("scores_")]:
    record_quantiles(key)
record_quantiles("gamma8193", quantiles=[0.9, 0.1, 0.5, 0.33])  # unsorted
record_quantiles("gamma257", quantiles=[0.5, 0.25, 0.5, 1.0, 0.25])  # duplicated
record_quantiles("mixed", quantiles=[0.3, 0.25])
record_quantiles("gamma256", quantiles=list(np.linspace(0.0, 1.0, 21)))  # more than one select call holds
record_quantiles("gamma10", add_newlines=False)
record_quantiles("zeros90", quantiles=[0.95, 0.05], add_newlines=False)
out["quantile_cases"] = np.array(quantile_cases)
record_error("cscores_quantiles", ref_rocco.cscores_quantiles, np.zeros(0), "empty")
record_error("cscores_quantiles", ref_rocco.cscores_quantiles, out["scores_gamma10"], "gamma10", quantiles=[0.5, 1.5])
record_error("cscores_quantiles", ref_rocco.cscores_quantiles, out["scores_gamma10"], "gamma10", quantiles=[-0.25])

# ---- z vectors: null scale, standardized scores, candidate masks ---------------------------------------------------
gen = np.random.default_rng(382443)


def z_vector(n, decimals, shift=0.0):
    return np.round(gen.normal(shift, 1.7, size=n), decimals) + 0.0


z = {
    "one_negative": np.array([-1.5]),
    "one_positive": np.array([2.5]),
    "two": np.array([-0.5, 3.0]),
    "seven": z_vector(7, 1),
    "n64": z_vector(64, 0),
    "n299": z_vector(299, 2),
    "n1000": z_vector(1000, 3, 0.4),
    "n8193": z_vector(8193, 2),
    "positive_odd": np.abs(z_vector(255, 2)) + 0.01,
    "positive_even": np.abs(z_vector(256, 2)) + 0.01,
    "zeros": np.zeros(33),
}
dirty = z_vector(300, 1)
dirty[[4, 90]] = np.nan
dirty[[7, 150, 151]] = np.inf
dirty[[9, 200]] = -np.inf
z["non_finite"] = dirty
rest = np.abs(z_vector(100, 1)) + 0.5
rest[[0, 50]] = -np.inf
rest[10] = np.nan
z["positive_with_minus_inf"] = rest  # no finite score <= 0: the fall-back, with -inf below the finite scores
mask_cases = []
for key, vector in z.items():
    out[f"z_{key}"] = vector
    standardized, null_scale = ref_inference._standardize_wls_z_scores(vector)
    assert standardized.dtype == np.float64 and isinstance(null_scale, float)
    out[f"standardized_{key}"] = standardized
    for tail_z, min_signal in ((2.0, 0.0), (0.5, 0.0), (3.0, 0.0), (2.0, 1.5), (1.0, 0.3)):
        mask = ref_inference.candidate_mask_from_wls(vector, tail_z=tail_z, min_signal=min_signal)
        assert mask.dtype == np.bool_
        out[f"mask_{len(mask_cases)}"] = mask
        mask_cases.append(json.dumps({"z": key, "tail_z": tail_z, "min_signal": min_signal, "null_scale": null_scale}))
out["mask_cases"] = np.array(mask_cases)
record_error("_standardize_wls_z_scores", ref_inference._standardize_wls_z_scores, np.array([np.nan, np.inf, -np.inf]), "all_non_finite")
record_error("candidate_mask_from_wls", ref_inference.candidate_mask_from_wls, np.array([np.nan, np.inf]), "all_non_finite")
record_error("_standardize_wls_z_scores", ref_inference._standardize_wls_z_scores, np.zeros(0), "empty")
record_error("_standardize_wls_z_scores", ref_inference._standardize_wls_z_scores, np.zeros((2, 3)), "two_dimensional")
record_error("candidate_mask_from_wls", ref_inference.candidate_mask_from_wls, np.zeros((2, 3)), "two_dimensional")

scale_cases = []
values = {"empty": np.zeros(0), "n1": np.array([4.0]), "even": z_vector(100, 2), "odd": z_vector(101, 2), "with_inf": dirty[np.isfinite(dirty) | np.isinf(dirty)],
          "with_nan": dirty, "constant": np.full(17, 3.5), "mostly_inf": np.array([np.inf, np.inf, np.inf, 1.0, 2.0])}
for key, vector in values.items():
    out[f"values_{key}"] = vector
    for floor in (1.0e-6, 0.5):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            result = ref_inference._robust_scale(vector, floor=floor)
        assert isinstance(result, float)
        scale_cases.append(json.dumps({"values": key, "floor": floor, "result": result}))
out["scale_cases"] = np.array(scale_cases)

# ---- p vectors: Benjamini-Hochberg masks -----------------------------------------------------------------------------
gen = np.random.default_rng(382400)
p = {
    "one_passing": np.array([0.001]),
    "one_failing": np.array([0.6]),
    "all_passing": np.round(gen.random(50) * 1.0e-4, 6),
    "none_passing": 0.5 + 0.5 * gen.random(64),
    "ties_2dp": np.round(gen.random(399) ** 3, 2),
    "ties_6dp": np.round(gen.random(1000) ** 4, 6),
    "n8193": np.round(gen.random(8193) ** 6, 3),
}
with_nan = np.round(gen.random(300) ** 3, 2)
with_nan[[2, 40, 299]] = np.nan
p["with_nan"] = with_nan
# ties exactly at the cutoff: ranks 3..6 (1-based) all hold 0.05 and only the last of them passes 0.1 * k / 10 on its own
p["ties_at_cutoff"] = np.array([0.9, 0.05, 0.001, 0.05, 0.8, 0.05, 0.002, 0.05, 0.7, 0.95])
# NaNs with the sign bit set (what 0.0 / 0.0 gives on x86-64): np.argsort puts them last like any NaN, a sort of bit patterns
# puts them first, where each would lift every real p-value one rank.  0.03 alone among two fails 0.05 * 1 / 2 but would
# pass 0.05 * 2 / 2; the longer vectors mix both signs of NaN around cutoffs that an offset of three ranks moves.
minus_nan = np.copysign(np.nan, -1.0)
p["minus_nan_at_cutoff"] = np.array([minus_nan, 0.03])
p["minus_nan_only"] = np.array([minus_nan, minus_nan])
both_nans = p["ties_2dp"].copy()
both_nans[[0, 17, 200]] = minus_nan
both_nans[[5, 300]] = np.nan
p["both_nans"] = both_nans
p["minus_nan_ties_at_cutoff"] = np.concatenate((p["ties_at_cutoff"], [minus_nan, minus_nan, minus_nan]))
assert all(np.signbit(v[np.isnan(v)]).any() for k, v in p.items() if "minus_nan" in k or k == "both_nans")
bh_cases = []
for key, vector in p.items():
    out[f"p_{key}"] = vector
    for fdr in (0.01, 0.05, 0.1, 0.2, 0.5):
        mask = ref_inference.benjamini_hochberg(vector, fdr=fdr)
        assert mask.dtype == np.bool_
        out[f"bh_mask_{len(bh_cases)}"] = mask
        bh_cases.append(json.dumps({"p": key, "fdr": fdr, "passing": int(mask.sum())}))
mask = ref_inference.benjamini_hochberg(np.zeros(0))
assert mask.dtype == np.bool_ and mask.shape == (0,)
out["bh_cases"] = np.array(bh_cases)
record_error("benjamini_hochberg", ref_inference.benjamini_hochberg, np.zeros((2, 3)), "two_dimensional")

out["errors"] = np.array(errors)
path = os.path.join(HERE, "locus_summaries_vectors.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {len(quantile_cases)} quantile, {len(mask_cases)} mask, {len(scale_cases)} scale, {len(bh_cases)} BH cases, "
      f"{len(errors)} errors, {os.path.getsize(path) / 1e3:.0f} kB")
