"""Post-hoc peak scoring (rocco/scores.py).  Two halves, both on the device:

* the arithmetic after the counting (rocco/scores.py:120-149, 180-194, 560-625) -- the signal statistic, its survival
  under the empirical null of the peak's length bin, Benjamini-Hochberg q-values, the narrowPeak columns (peakscore.hip);
  the last three formatting statements (-log10, rounding to four decimals, the UCSC score) are NumPy calls on the short
  per-peak vectors, as in the reference;
* the counting itself for records already decoded (interval_count.hip): reads per peak per
  file (`raw_count_matrix_from_records`, rocco/scores.py:250-341), reads per random background region per file
  (`get_ecdf_from_records` / `multi_ecdf_from_records`, rocco/scores.py:642-785) and the composition
  (`score_peaks_from_records`, rocco/scores.py:381-639), for a caller that brings the records and the whole-file facts
  (mapped reads, read length);
* the same functions over BAM paths under the reference's names and signatures:
  `raw_count_matrix`, `get_read_length`, `score_peaks`, `get_ecdf`, `multi_ecdf`.  Files come from
  `rocco_amd.bam._cached_file`, the whole-file facts from the index statistics and decoded heads, and the counting goes
  contig group by contig group (`_count_paths`), peaks and null regions of a group in one call.
"""
from __future__ import annotations

import ctypes
import logging
import os
from collections import OrderedDict
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import _native
from . import bam as _bam
from . import dp as _dp
from . import readtracks as _readtracks

logger = logging.getLogger(__name__)


class EmpiricalNull:
    """Finite-sample empirical null of one length bin (rocco/scores.py:120-149): right-tail survival with a plus-one
    correction, and the plain empirical CDF."""

    def __init__(self, values):
        ordered = np.sort(np.asarray(values, dtype=np.float64))
        if ordered.ndim != 1 or ordered.size == 0:
            raise ValueError("`values` must be a non-empty one-dimensional array.")
        self.values, self.size = ordered, int(ordered.size)

    def survival(self, x):
        x_ = np.asarray(x, dtype=np.float64)
        below = np.searchsorted(self.values, x_, side="left")
        out = (self.size - below + 1.0) / (self.size + 1.0)
        return float(out) if x_.ndim == 0 else out

    def evaluate(self, x):
        x_ = np.asarray(x, dtype=np.float64)
        out = np.searchsorted(self.values, x_, side="right") / float(self.size)
        return float(out) if x_.ndim == 0 else out


def _device(arr, dtype):
    import torch

    if _dp._is_tensor(arr):
        t = arr if arr.is_cuda else arr.to(f"cuda:{_dp._device_index()}")
        return t.to(dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(f"cuda:{_dp._device_index()}").to(dtype).contiguous()


def peak_signal_stat_device(counts_t, lengths_t, row_scale: float = 1000.0, pc: float = 1.0, percentile: float = 75.0):
    """`_peak_signal_stat` (rocco/scores.py:180-194) of every row of a [peaks, samples] float64 CUDA tensor."""
    import torch

    P, K = int(counts_t.shape[0]), int(counts_t.shape[1])
    out = torch.empty(P, dtype=torch.float64, device=counts_t.device)
    solver = _native.solver_for(counts_t.device.index)
    _native.check(_native.load().rocco_hip_peak_signal_stat_f64(
        solver.handle, counts_t.data_ptr(), lengths_t.data_ptr(), P, K, float(row_scale), float(pc), float(percentile),
        out.data_ptr(), _dp._stream_ptr(counts_t)), "rocco_hip_peak_signal_stat_f64")
    return out


def _peak_signal_stat(vals, length, row_scale: float = 1000.0, pc: float = 1.0, percentile: float = 75.0) -> float:
    """Same call as the reference's helper, for one peak."""
    import torch

    counts = _device(np.asarray(vals, dtype=np.float64).reshape(1, -1), torch.float64)
    lengths = _device(np.array([float(length)]), torch.float64)
    return float(peak_signal_stat_device(counts, lengths, row_scale, pc, percentile)[0])


def benjamini_hochberg_device(pvals_t):
    """scipy.stats.false_discovery_control(ps, method="bh") (rocco/scores.py:583) on a float64 CUDA tensor.  As SciPy, a
    NaN or a value outside [0, 1] is refused (one reduction on the device, read back before the kernels are queued)."""
    import torch

    m = int(pvals_t.shape[0])
    if m > 0 and not bool(((pvals_t >= 0.0) & (pvals_t <= 1.0)).all()):  # (a NaN fails both comparisons)
        raise ValueError("`ps` must include only numbers between 0 and 1.")
    if m <= 1:
        return pvals_t.clone()
    out = torch.empty_like(pvals_t)
    solver = _native.solver_for(pvals_t.device.index)
    _native.check(_native.load().rocco_hip_bh_adjust_f64(solver.handle, pvals_t.data_ptr(), m, out.data_ptr(), _dp._stream_ptr(pvals_t)),
                  "rocco_hip_bh_adjust_f64")
    return out


def score_peak_counts(count_matrix, lengths, binned_lengths, ecdf_dict: Dict[int, EmpiricalNull], row_scale: float = 1000.0,
                      pc: float = 1.0, ucsc_base: int = 250) -> dict:
    """Everything `score_peaks` computes after its counting and scaling (rocco/scores.py:560-625).

    `count_matrix`: [peaks, samples] scaled counts; `lengths`: peak lengths in bp; `binned_lengths[p]`: the key of the
    peak's length bin in `ecdf_dict` (`_assign_length_bins`); `ecdf_dict[key]`: the bin's EmpiricalNull (or its values).
    Returns the arrays the reference writes: signal values, p-values, q-values, the UCSC score column and the rounded
    -log10 columns."""
    import torch

    counts_t = _device(count_matrix, torch.float64)
    if counts_t.dim() != 2:
        raise ValueError("`count_matrix` must be two-dimensional (peaks x samples)")
    P = int(counts_t.shape[0])
    lengths_h = np.asarray(lengths, dtype=np.float64)
    if lengths_h.shape != (P,):
        raise ValueError("`lengths` must hold one entry per peak")
    keys = sorted(ecdf_dict)
    position = {int(k): i for i, k in enumerate(keys)}
    nulls = [np.sort(np.asarray(getattr(ecdf_dict[k], "values", ecdf_dict[k]), dtype=np.float64)) for k in keys]
    if any(v.size == 0 for v in nulls):
        raise ValueError("`values` must be a non-empty one-dimensional array.")
    offsets = np.concatenate([[0], np.cumsum([v.size for v in nulls])]).astype(np.int64)
    bins_h = np.array([position[int(b)] for b in np.asarray(binned_lengths)], dtype=np.int32)
    sig_t = peak_signal_stat_device(counts_t, _device(lengths_h, torch.float64), row_scale, pc)
    pvals_t = torch.empty_like(sig_t)
    solver = _native.solver_for(counts_t.device.index)
    null_t, off_t, bin_t = _device(np.concatenate(nulls), torch.float64), _device(offsets, torch.int64), _device(bins_h, torch.int32)
    _native.check(_native.load().rocco_hip_ecdf_survival_f64(solver.handle, sig_t.data_ptr(), bin_t.data_ptr(), null_t.data_ptr(),
                                                             off_t.data_ptr(), P, pvals_t.data_ptr(), _dp._stream_ptr(sig_t)),
                  "rocco_hip_ecdf_survival_f64")
    qvals_t = benjamini_hochberg_device(pvals_t)
    sig, pvals, qvals = sig_t.cpu().numpy(), pvals_t.cpu().numpy(), qvals_t.cpu().numpy()
    # narrowPeak columns (rocco/scores.py:604-616): NumPy on the per-peak vectors, as the reference
    bed6 = np.minimum(np.array(ucsc_base + sig / np.quantile(sig, q=0.99) * (1000 - ucsc_base), dtype=int), 1000)
    return {"signal": sig, "pvals": pvals, "qvals": qvals, "bed6_scores": bed6,
            "signal_out": np.round(sig, 4), "pvals_out": np.round(-np.log10(pvals + 1e-10), 4),
            "qvals_out": np.round(-np.log10(qvals + 1e-10), 4)}


def write_scored_peaks(bed_strings: Sequence[str], names: Sequence[str], lengths, scored: dict, output_file: str,
                       summit_offsets: Optional[Dict[str, int]] = None) -> str:
    """The narrowPeak-like rows `score_peaks` writes (rocco/scores.py:618-637)."""
    offsets = summit_offsets or {}
    with open(output_file, "w") as fh:
        for i, peak in enumerate(bed_strings):
            summit = int(offsets.get(names[i], -1))
            if summit >= 0:
                summit = int(np.clip(summit, 0, max(int(lengths[i]) - 1, 0)))
            fh.write(f"{peak}\t{names[i]}\t{scored['bed6_scores'][i]}\t.\t{scored['signal_out'][i]}\t"
                     f"{scored['pvals_out'][i]}\t{scored['qvals_out'][i]}\t{summit}\n")
    return output_file


# --------------------------------------------------------------------------------------------
# the counting half for decoded records (csrc/interval_count.hip)
# --------------------------------------------------------------------------------------------

RAW_COUNT_OPTIONS = dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10)   # rocco/scores.py:314-324
# pysam's AlignmentFile.count(chrom, start, end, read_callback=_check_read) (rocco/scores.py:152-161, 706-711): the
# records the index iterator yields that are mapped and have mapq >= 10.  The same iterator, the same filters, and the
# unshifted read overlaps the region exactly when the iterator yields it: the counter's rule at these options (argued,
# not run against pysam).
NULL_COUNT_OPTIONS = dict(one_read_per_bin=1, flag_exclude=4, min_mapping_quality=10)


def _random_intervals(chrom_sizes_file: str, length: int, nsamples: int, seed=None) -> list:
    """rocco/scores.py:38-77, the same NumPy calls in the same order (the generator stream is the reference's)."""
    chrom_sizes = _readtracks.get_chroms_and_sizes(chrom_sizes_file)
    length_ = int(max(1, length))
    chroms, max_starts = [], []
    for chrom, chrom_size in chrom_sizes.items():
        max_start = int(chrom_size) - length_ + 1
        if max_start <= 0:
            continue
        chroms.append(str(chrom))
        max_starts.append(int(max_start))
    if len(chroms) == 0:
        raise ValueError(f"No chromosome in {chrom_sizes_file} is long enough for intervals of length {length_}.")
    weights = np.asarray(max_starts, dtype=np.float64)
    weight_sum = float(np.sum(weights))
    if not np.isfinite(weight_sum) or weight_sum <= 0.0:
        raise ValueError("Could not construct a valid random-interval sampler.")
    weights = weights / weight_sum
    rng = np.random.default_rng(seed)
    chrom_indices = rng.choice(len(chroms), size=int(max(1, nsamples)), replace=True, p=weights)
    starts = [int(rng.integers(0, max_starts[int(chrom_idx)])) for chrom_idx in chrom_indices]
    return [(chroms[int(chrom_idx)], int(start), int(start + length_)) for chrom_idx, start in zip(chrom_indices, starts)]


def _read_peak_intervals(peak_file: str, min_columns: int = 3):
    """rocco/scores.py:89-117: (chroms, starts, ends, bed_strings, names) of a BED file."""
    chroms, starts, ends, bed_strings, names = [], [], [], [], []
    with open(peak_file, encoding="utf-8") as handle:
        for line_num, line in enumerate(handle, start=1):
            line_ = line.strip()
            if line_ == "":
                continue
            fields = line_.split("\t")
            if len(fields) < int(max(3, min_columns)):
                raise ValueError(f"Peak file row {line_num} has fewer than {max(3, min_columns)} columns.")
            chroms.append(str(fields[0]))
            starts.append(int(fields[1]))
            ends.append(int(fields[2]))
            bed_strings.append("\t".join(fields[0:3]))
            names.append("_".join(fields[0:3]))
    return chroms, starts, ends, bed_strings, names


def _null_stat(vals, percentile: float = 75.0):
    """rocco/scores.py:164-173."""
    return np.percentile(vals, percentile)


def _assign_length_bins(lengths, max_bins: int = 24, min_bin_width_bp: int = 100):
    """rocco/scores.py:195-247: (the representative length of every peak's bin, the sorted representatives)."""
    lengths_ = np.maximum(np.asarray(lengths, dtype=np.int64), 1)
    if lengths_.ndim != 1 or lengths_.size == 0:
        raise ValueError("`lengths` must be a non-empty one-dimensional array.")
    uniq_lengths = np.unique(lengths_)
    span_bp = int(uniq_lengths[-1] - uniq_lengths[0])
    width_limited_max_bins = 1
    if span_bp >= int(min_bin_width_bp):
        width_limited_max_bins = max(1, span_bp // int(min_bin_width_bp))
    effective_max_bins = max(1, min(int(max_bins), int(width_limited_max_bins)))
    if uniq_lengths.size <= effective_max_bins:
        return lengths_.astype(np.int64, copy=False), uniq_lengths.astype(np.int64, copy=False)
    log_edges = np.linspace(np.log(float(uniq_lengths[0])), np.log(float(uniq_lengths[-1])), num=int(effective_max_bins) + 1)
    bin_ids = np.digitize(np.log(uniq_lengths.astype(np.float64)), log_edges[1:-1], right=False)
    length_to_bin, bin_representatives = {}, []
    for bin_id in np.unique(bin_ids):
        members = uniq_lengths[bin_ids == bin_id]
        representative = max(int(np.median(members)), 1)
        bin_representatives.append(representative)
        for length in members:
            length_to_bin[int(length)] = representative
    binned_lengths = np.asarray([length_to_bin[int(length)] for length in lengths_], dtype=np.int64)
    return binned_lengths, np.asarray(sorted(set(bin_representatives)), dtype=np.int64)


def _interval_counts_device(records_by_file: Sequence[dict], chroms, starts, ends, files_per_call: Optional[int], **options):
    """int32 CUDA tensor [P, F]: `count_alignment_intervals_batch_device` over ``files_per_call`` files at a time (all of
    them by default).  Counting is independent per file; a call holds 16 bytes per record of its files on the device."""
    import torch

    F = len(records_by_file)
    if F == 0:
        raise ValueError("no files")
    if files_per_call is None:
        per_call = F
    else:
        per_call = int(files_per_call)
        if per_call < 1:
            raise ValueError("`files_per_call` must be at least 1")
    parts = [_readtracks.count_alignment_intervals_batch_device(records_by_file[f: f + per_call], chroms, starts, ends, **options)
             for f in range(0, F, per_call)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _reference_count_matrix(counts: np.ndarray) -> np.ndarray:
    """The reference's float32 per interval is min(count, 2**24); np.rint(...).astype(np.int64) of it."""
    return np.minimum(counts, _readtracks.EXACT_COUNT_LIMIT).astype(np.int64)


def _write_count_matrix(output_file: str, sample_names: Sequence[str], peak_names: Sequence[str], count_matrix: np.ndarray) -> str:
    """The TSV of rocco/scores.py:333-339: header ``peak_name`` + samples, one row of integer counts per peak."""
    with open(output_file, "w", encoding="utf-8") as handle:
        handle.write("peak_name\t" + "\t".join(str(name) for name in sample_names) + "\n")
        for peak_idx, peak_name in enumerate(peak_names):
            handle.write(f"{peak_name}\t" + "\t".join(str(int(value)) for value in count_matrix[peak_idx]) + "\n")
    return output_file


def raw_count_matrix_from_records(records_by_file: Sequence[dict], sample_names: Sequence[str], peak_file: str, output_file: str,
                                  bed_columns: int = 3, files_per_call: Optional[int] = None) -> str:
    """``raw_count_matrix`` (rocco/scores.py:250-341) for decoded records: ``records_by_file[f]`` is ``{contig:
    AlignmentRecords}`` of sample ``sample_names[f]`` (the reference's name is the BAM's base name without ``.bam``).
    Writes the reference's TSV bytes (header ``peak_name`` + samples, one row of integer counts per peak) and returns
    ``output_file``.  All peaks and files are counted in one launch series (the reference loops over both)."""
    if len(sample_names) != len(records_by_file):
        raise ValueError("one sample name per file is required")
    chroms, starts, ends, _, peak_names = _read_peak_intervals(peak_file, min_columns=bed_columns)
    if len(peak_names) == 0:
        raise ValueError("Peak file does not contain any intervals.")
    counts = _interval_counts_device(records_by_file, chroms, starts, ends, files_per_call, **RAW_COUNT_OPTIONS).cpu().numpy()
    if output_file is not None and os.path.exists(output_file):
        os.remove(output_file)
    return _write_count_matrix(output_file, sample_names, peak_names, _reference_count_matrix(counts))


def _scaling_constants(sample_scaling_constants, F: int) -> np.ndarray:
    constants = (np.ones(F, dtype=np.float64) if sample_scaling_constants is None
                 else np.asarray(sample_scaling_constants, dtype=np.float64))
    if constants.shape[0] != F:
        raise ValueError("`sample_scaling_constants` must match the number of BAM files.")
    return constants


def _nulls_from_counts(counts_t, length: int, constants: np.ndarray, null_stat, trim_proportion: float, row_scale: float, pc: float):
    """rocco/scores.py:702-733 from the [nsamples, F] counts of one length bin."""
    import torch

    scaled_t = counts_t.to(torch.float64) * _device(constants, torch.float64)  # count * sample_scaling_constants_[j]
    length_ = max(int(length), 1)
    if null_stat is _null_stat:
        # np.percentile(log2(max(cperlen * (row_scale / length) + pc, pc)), 75): `_peak_signal_stat`'s expression
        lengths_t = torch.full((int(scaled_t.shape[0]),), float(length_), dtype=torch.float64, device=scaled_t.device)
        len_avgs = peak_signal_stat_device(scaled_t.contiguous(), lengths_t, float(row_scale), float(pc), 75.0).cpu().numpy()
    else:
        cperlen = scaled_t.cpu().numpy()
        transformed = np.log2(np.maximum(cperlen * (float(row_scale) / float(length_)) + float(pc), float(pc)))
        len_avgs = np.array([null_stat(row) for row in transformed])
    if trim_proportion > 0:  # scipy.stats.trim1(len_avgs, proportiontocut=trim_proportion, tail="right")
        keep = len_avgs.shape[0] - int(trim_proportion * len_avgs.shape[0]) if trim_proportion < 1 else 0
        len_avgs = np.sort(len_avgs)[:keep]
    return EmpiricalNull(len_avgs)


def get_ecdf_from_records(records_by_file: Sequence[dict], length: int, chrom_sizes_file: str, nsamples=500,
                          sample_scaling_constants=None, seed=None, null_stat: Callable = _null_stat, trim_proportion: float = 0.0,
                          row_scale: float = 1000.0, pc: float = 1.0, files_per_call: Optional[int] = None) -> EmpiricalNull:
    """``get_ecdf`` (rocco/scores.py:642-733) for decoded records: the random regions of `_random_intervals` counted in
    one call at `NULL_COUNT_OPTIONS`, then the statistic of every region on the device (the default ``null_stat``; a
    caller's own callable gets the transformed rows on the host)."""
    constants = _scaling_constants(sample_scaling_constants, len(records_by_file))
    intervals = _random_intervals(chrom_sizes_file, length=int(length), nsamples=int(nsamples), seed=seed)
    counts_t = _interval_counts_device(records_by_file, [i[0] for i in intervals], [i[1] for i in intervals],
                                       [i[2] for i in intervals], files_per_call, **NULL_COUNT_OPTIONS)
    return _nulls_from_counts(counts_t, length, constants, null_stat, trim_proportion, row_scale, pc)


def multi_ecdf_from_records(records_by_file: Sequence[dict], lengths, chrom_sizes_file: str, nsamples_per_length,
                            sample_scaling_constants=None, seed=None, null_stat: Callable = _null_stat, row_scale: float = 1000.0,
                            pc: float = 1.0, files_per_call: Optional[int] = None) -> "OrderedDict":
    """``multi_ecdf`` (rocco/scores.py:741-785): one `EmpiricalNull` per unique representative length.  The reference runs
    one `get_ecdf` per length under a process pool; here the random regions of ALL lengths go to the device in one
    counting call."""
    np.random.seed(seed)  # (as the reference, :757)
    constants = _scaling_constants(sample_scaling_constants, len(records_by_file))
    uniq_lengths, per_length = _null_intervals(lengths, chrom_sizes_file, nsamples_per_length, seed)
    everything = [interval for intervals in per_length for interval in intervals]
    counts_t = _interval_counts_device(records_by_file, [i[0] for i in everything], [i[1] for i in everything],
                                       [i[2] for i in everything], files_per_call, **NULL_COUNT_OPTIONS)
    return _nulls_by_length(counts_t, uniq_lengths, per_length, constants, null_stat, row_scale, pc)


def _null_intervals(lengths, chrom_sizes_file: str, nsamples_per_length, seed):
    """(the unique representative lengths, the random regions `get_ecdf` draws for each of them)"""
    uniq_lengths = np.unique(lengths)
    return uniq_lengths, [_random_intervals(chrom_sizes_file, length=int(length), nsamples=int(nsamples_per_length), seed=seed)
                          for length in uniq_lengths]


def _nulls_by_length(counts_t, uniq_lengths, per_length, constants, null_stat, row_scale, pc) -> "OrderedDict":
    """One `EmpiricalNull` per length from the [regions of all lengths, F] counts, the lengths' regions one behind the other."""
    out, at = OrderedDict(), 0
    for length, intervals in zip(uniq_lengths, per_length):
        out[length] = _nulls_from_counts(counts_t[at: at + len(intervals)], length, constants, null_stat, 0.0, row_scale, pc)
        at += len(intervals)
    return out


def _read_count_matrix(count_matrix_file: str) -> np.ndarray:
    """The ``.values`` of ``pd.read_csv(file, sep="\t", header=0, index_col=0)`` for a matrix `raw_count_matrix` wrote: int64
    when every cell is an integer (what the reference then scales IN that integer array), float64 otherwise."""
    with open(count_matrix_file, encoding="utf-8") as handle:
        rows = [line.rstrip("\n").split("\t")[1:] for line in handle if line.strip() != ""][1:]
    try:
        return np.array([[int(cell) for cell in row] for row in rows], dtype=np.int64)
    except ValueError:
        return np.array([[float(cell) for cell in row] for row in rows], dtype=np.float64)


def _scale_count_matrix(matrix_: np.ndarray, n_peaks: int, F: int, chrom_sizes_file, effective_genome_size, skip_for_norm,
                        mapped_counts, read_lengths) -> np.ndarray:
    """rocco/scores.py:499-533: the sample scaling constants, and the matrix scaled IN PLACE in its own dtype (NumPy casts
    the float64 products back: truncation toward zero for the int64 matrix pandas read).  Returns the constants."""
    if matrix_.shape != (n_peaks, F):
        raise ValueError("the count matrix does not hold one row per peak and one column per file")
    if effective_genome_size is None:
        effective_genome_size = np.sum([x[1] for x in _readtracks.get_chroms_and_sizes(chrom_sizes_file).items()
                                        if x[0] not in skip_for_norm])
    mapped_sizes = np.asarray(mapped_counts, dtype=int) * np.asarray(read_lengths, dtype=int)
    sample_scaling_constants = (effective_genome_size) / mapped_sizes
    for sample_idx in range(F):
        matrix_[:, sample_idx] = matrix_[:, sample_idx] * sample_scaling_constants[sample_idx]
    return sample_scaling_constants


def _read_summit_offsets(summit_offsets_file: Optional[str]) -> dict:
    """rocco/scores.py:595-607."""
    summit_offsets = {}
    if summit_offsets_file is not None:
        with open(summit_offsets_file, encoding="utf-8") as handle:
            for line_num, line in enumerate(handle, start=1):
                line_ = line.strip()
                if line_ == "":
                    continue
                fields = line_.split("\t")
                if len(fields) < 2:
                    raise ValueError(f"Summit offset row {line_num} in {summit_offsets_file} has fewer than 2 columns.")
                summit_offsets[str(fields[0])] = int(fields[1])
    return summit_offsets


def _score_and_write(matrix_, lengths, binned_lengths, ecdf_dict, bed_strings, names, row_scale, pc, ucsc_base,
                     summit_offsets_file, output_file):
    """rocco/scores.py:564-639 from the scaled matrix and the nulls: (signal values, UCSC scores, p-values); writes
    ``output_file``."""
    scored = score_peak_counts(matrix_.astype(np.float64), lengths, binned_lengths, ecdf_dict, row_scale=row_scale, pc=pc,
                               ucsc_base=ucsc_base)
    write_scored_peaks(bed_strings, names, lengths, scored, output_file, _read_summit_offsets(summit_offsets_file))
    return scored["signal"], scored["bed6_scores"], scored["pvals"]


def score_peaks_from_records(records_by_file: Sequence[dict], sample_names: Sequence[str], chrom_sizes_file: str, peak_file: str,
                             mapped_counts: Sequence[int], read_lengths: Sequence[int], count_matrix_file: Optional[str] = None,
                             effective_genome_size: Optional[float] = None, skip_for_norm: Sequence[str] = ("chrX", "chrY", "chrM"),
                             row_scale=1000, ucsc_base=250, pc=1, ecdf_nsamples=500, ecdf_max_length_bins: int = 24,
                             output_file="scored_peaks.bed", seed: Optional[int] = None, summit_offsets_file: Optional[str] = None,
                             files_per_call: Optional[int] = None):
    """``score_peaks`` (rocco/scores.py:381-639) for decoded records: counts over the peaks -> sample scaling constants ->
    the reference's in-place scaling -> length bins -> empirical nulls -> `score_peak_counts` -> `write_scored_peaks`.
    ``mapped_counts[f]`` (mapped reads outside ``skip_for_norm``, :514-520) and ``read_lengths[f]`` (`get_read_length`,
    :344-378) are the whole-file facts the reader supplies.  ``count_matrix_file``: read when it exists, else written (when
    given).  The reference scales the matrix inside the int64 array pandas read from the TSV (:528-533), which truncates
    every scaled count toward zero; that is reproduced.  As in the reference, the nulls always use the default statistic.
    Returns (signal values, UCSC scores, p-values) and writes ``output_file``."""
    F = len(records_by_file)
    if len(sample_names) != F or len(mapped_counts) != F or len(read_lengths) != F:
        raise ValueError("one sample name, mapped count and read length per file are required")
    chroms, starts, ends, bed_strings, names = _read_peak_intervals(peak_file, min_columns=3)
    if count_matrix_file is not None and os.path.exists(count_matrix_file):
        matrix_ = _read_count_matrix(count_matrix_file)
    else:
        if len(names) == 0:
            raise ValueError("Peak file does not contain any intervals.")
        counts = _interval_counts_device(records_by_file, chroms, starts, ends, files_per_call, **RAW_COUNT_OPTIONS).cpu().numpy()
        matrix_ = _reference_count_matrix(counts)
        if count_matrix_file is not None:
            _write_count_matrix(count_matrix_file, sample_names, names, matrix_)
    lengths = np.asarray([end - start for start, end in zip(starts, ends)], dtype=np.float64)
    sample_scaling_constants = _scale_count_matrix(matrix_, len(names), F, chrom_sizes_file, effective_genome_size, skip_for_norm,
                                                   mapped_counts, read_lengths)
    binned_lengths, ecdf_lengths = _assign_length_bins(lengths, max_bins=ecdf_max_length_bins)
    if seed is None:
        seed = np.random.randint(1, 10000)
    ecdf_dict = multi_ecdf_from_records(records_by_file, ecdf_lengths, chrom_sizes_file, nsamples_per_length=ecdf_nsamples,
                                        sample_scaling_constants=sample_scaling_constants, seed=seed, row_scale=row_scale, pc=pc,
                                        files_per_call=files_per_call)
    return _score_and_write(matrix_, lengths, binned_lengths, ecdf_dict, bed_strings, names, row_scale, pc, ucsc_base,
                            summit_offsets_file, output_file)


# --------------------------------------------------------------------------------------------
# the same functions over BAM paths (note (33)): the reference's signatures
# --------------------------------------------------------------------------------------------

# Decoded records of one contig group, summed over the files, at 20 bytes per record (the alignment cache's measure).  Half
# of the cache's budget, so that a group and the copy the counter takes of it fit together: a choice, not a measurement
# (DESIGN.md note (33)).
GROUP_BYTES = _bam.ALIGNMENT_CACHE_BYTES // 2
_DEFAULT_SKIP_FOR_NORM = ["chrX", "chrY", "chrM"]


def _contig_groups(contigs: Sequence[str], costs: Sequence[Optional[int]], budget: int) -> list:
    """Runs of ``contigs`` (kept in their order) whose costs add up to ``budget`` at most; a contig above the budget, or of
    unknown cost (None), is a group of its own."""
    groups, run, total = [], [], 0
    for contig, cost in zip(contigs, costs):
        alone = cost is None or int(cost) > budget
        if run and (alone or total + int(cost) > budget):
            groups.append(run)
            run, total = [], 0
        if alone:
            groups.append([contig])
            continue
        run.append(contig)
        total += int(cost)
    if run:
        groups.append(run)
    return groups


def _sample_names(bam_files: Sequence[str]) -> list:
    """rocco/scores.py:291-296: the base name without ``.bam``."""
    samples = []
    for bam in bam_files:
        name = os.path.basename(bam)
        if name.endswith(".bam"):
            name = name[:-4]
        samples.append(name)
    return samples


def _open_files(bam_files) -> tuple:
    bam_files_ = _readtracks.check_type_bam_files(bam_files)
    return bam_files_, [_bam._cached_file(path) for path in bam_files_]


def _known_records(file, contig: str) -> Optional[int]:
    """The records of a contig by what is known without decoding: ``count(contig)`` of an indexed file (None where the index
    has no statistics for it), the track length of a resident file."""
    count = getattr(file, "count", None)
    return count(contig) if count is not None else len(file.records[contig])


def _count_paths(files: Sequence, families: Sequence[tuple], files_per_call: Optional[int] = None):
    """int32 CUDA tensor [P_total, F]: the counts of one or two interval families over the files (`_cached_file`), rows in
    the caller's order (the families one behind the other).  ``families[s] = (chroms, starts, ends, options)``.  The pass
    goes contig group by contig group (`_contig_groups` under `GROUP_BYTES`): a group's (file, contig) pairs are fetched
    with ONE `_load_contigs` call and counted with ONE `count_alignment_intervals_sets_device` call per column group of
    ``files_per_call`` files (all files by default), every family under its own option set, into the final rows.  Contigs
    without intervals are never decoded; a file without an index is resident as a whole and goes through the same call."""
    import torch

    F = len(files)
    if F == 0:
        raise ValueError("no files")
    if files_per_call is None:
        per_call = F
    else:
        per_call = int(files_per_call)
        if per_call < 1:
            raise ValueError("`files_per_call` must be at least 1")
    chroms, starts, ends, sets = [], [], [], []
    for s, (chroms_s, starts_s, ends_s, _) in enumerate(families):
        chroms_s, starts_s, ends_s = _readtracks._check_intervals(chroms_s, starts_s, ends_s)
        chroms += chroms_s
        starts.append(starts_s)
        ends.append(ends_s)
        sets.append(np.full(len(chroms_s), s, dtype=np.int32))
    option_sets = [dict(family[3]) for family in families]
    starts_h, ends_h, sets_h = np.concatenate(starts), np.concatenate(ends), np.concatenate(sets)
    chroms_h = np.asarray(chroms, dtype=object)
    P = len(chroms)
    wanted = list(dict.fromkeys(chroms))
    for file in files:
        for contig in wanted:
            if contig not in file.records:
                raise ValueError("chromosome not found in alignment header")
    dev = _dp._device(None)
    out = torch.empty((P, F), dtype=torch.int32, device=dev)  # (every cell is addressed by exactly one call)
    if P == 0:
        return out
    header_order = {name: k for k, (name, _) in enumerate(files[0].contigs)}
    wanted.sort(key=lambda contig: header_order[contig])
    costs = []
    for contig in wanted:
        counts = [_known_records(file, contig) for file in files]
        costs.append(None if any(c is None for c in counts) else 20 * int(sum(counts)))
    indexed = [f for f, file in enumerate(files) if isinstance(file, _bam.IndexedAlignmentFile)]
    for group in _contig_groups(wanted, costs, int(GROUP_BYTES)):
        records = [dict() for _ in range(F)]
        if indexed:
            pairs = [(files[f], contig) for f in indexed for contig in group]
            for (file_, contig), track in zip(((f, c) for f in indexed for c in group), _bam._load_contigs(pairs)):
                records[file_][contig] = track
        for f in range(F):
            if f not in indexed:
                records[f] = {contig: files[f].records[contig] for contig in group}
        rows = np.flatnonzero(np.isin(chroms_h, group))
        for f0 in range(0, F, per_call):
            _readtracks.count_alignment_intervals_sets_device(records[f0: f0 + per_call], chroms_h[rows].tolist(), starts_h[rows],
                                                              ends_h[rows], sets_h[rows], option_sets, rows, out, col0=f0)
    return out


def _peak_family(chroms, starts, ends) -> tuple:
    return (chroms, starts, ends, RAW_COUNT_OPTIONS)


def _null_family(intervals) -> tuple:
    return ([i[0] for i in intervals], [i[1] for i in intervals], [i[2] for i in intervals], NULL_COUNT_OPTIONS)


def _log_count_matrix_start(sample_names, n_peaks: int, bam_files) -> None:
    """The INFO lines of rocco/scores.py:297-313 (the reference counts file by file; here all files are one pass)."""
    header = "peak_name\t" + "\t".join(sample_names)
    logger.info(f"\n\nCount matrix header: {header}\n\n")
    logger.info("Counting %s peak regions across %s alignments.", int(n_peaks), int(len(bam_files)))
    for sample_idx, bam_file in enumerate(bam_files):
        logger.info("Counting sample %s of %s: %s", sample_idx + 1, len(bam_files), bam_file)


def _finish_count_matrix(output_file: str, sample_names, peak_names, counts_t) -> np.ndarray:
    """rocco/scores.py:325-341 from the device counts: the int64 matrix, written to ``output_file``."""
    count_matrix = _reference_count_matrix(counts_t.cpu().numpy())
    if output_file is not None and os.path.exists(output_file):
        logger.warning(f"{output_file} already exists...overwriting.")
        os.remove(output_file)
    _write_count_matrix(output_file, sample_names, peak_names, count_matrix)
    logger.info("Count matrix written to %s", output_file)
    return count_matrix


def raw_count_matrix(bam_files, peak_file: str, output_file: str, bed_columns: int = 3, overwrite=True,
                     files_per_call: Optional[int] = None) -> str:
    """``raw_count_matrix`` (rocco/scores.py:250-341) over BAM paths: a list of paths or a text file naming them.  Returns
    ``output_file``.  (``overwrite`` is accepted and, as in the reference, not read.)"""
    bam_files_, files = _open_files(bam_files)
    chroms, starts, ends, _, peak_names = _read_peak_intervals(peak_file, min_columns=bed_columns)
    if len(peak_names) == 0:
        raise ValueError("Peak file does not contain any intervals.")
    samples = _sample_names(bam_files_)
    _log_count_matrix_start(samples, len(peak_names), bam_files_)
    counts_t = _count_paths(files, [_peak_family(chroms, starts, ends)], files_per_call)
    _finish_count_matrix(output_file, samples, peak_names, counts_t)
    return output_file


def _qualifies_for_read_length(flag: np.ndarray, mapq: np.ndarray, min_mapping_quality: int) -> np.ndarray:
    """rocco/scores.py:366-374: not unmapped, secondary or supplementary, and mapping quality at least the floor."""
    return ((np.asarray(flag).astype(np.int64) & (4 | 256 | 2048)) == 0) & (np.asarray(mapq).astype(np.int64) >= int(min_mapping_quality))


def _read_length_value(lengths: np.ndarray, name: str) -> int:
    """``int(np.percentile(read_lengths, 75))`` (rocco/scores.py:378) of the ``qlen`` taken.  pysam's ``infer_query_length()``
    is None for a query length of zero, and the list may be empty: NumPy refuses both, and the exception keeps its type
    with a message that names the file."""
    taken = [int(v) if int(v) != 0 else None for v in np.asarray(lengths).tolist()]
    try:
        return int(np.percentile(taken, 75))
    except Exception as error:
        why = "no read qualifies" if len(taken) == 0 else "a qualifying read has no query length (no CIGAR)"
        raise type(error)(f"get_read_length: {name}: {why}: {error}") from error


def read_length_from_fields(flag, mapq, qlen, num_reads: int = 1000, min_mapping_quality: int = 10, name: str = "") -> int:
    """`get_read_length` as a function of the records' fields in the order ``fetch()`` yields them (the header's contigs one
    behind the other, every contig in the index iterator's order)."""
    keep = _qualifies_for_read_length(flag, mapq, min_mapping_quality)
    return _read_length_value(np.asarray(qlen)[keep][: max(int(num_reads), 1)], name)


def _read_lengths(files: Sequence, num_reads: int = 1000, min_mapping_quality: int = 10) -> list:
    """`get_read_length` of every file.  An indexed file is read contig by contig in header order until ``num_reads``
    records qualify; per turn the next non-empty contig of EVERY file that is still short is fetched, in ONE `_load_contigs`
    call.  Of a contig the probe downloads a head (`_head_chunks`), not whole arrays."""
    quota = max(int(num_reads), 1)  # (the reference appends, then tests ``>= num_reads``: at least one read is taken)
    taken = [[] for _ in files]
    have = [0] * len(files)

    def probe(f, tracks):
        for chunk in _readtracks._head_chunks(tracks, ("flag", "mapq", "qlen"), first=max(quota, 1024)):
            good = chunk["qlen"][_qualifies_for_read_length(chunk["flag"], chunk["mapq"], min_mapping_quality)][: quota - have[f]]
            taken[f].append(good)
            have[f] += good.size
            if have[f] >= quota:
                return

    cursors = {}
    for f, file in enumerate(files):
        if isinstance(file, _bam.IndexedAlignmentFile):
            cursors[f] = iter([name for name, _ in file.contigs if file.count(name) != 0])
        else:
            tracks = file.tracks()
            _readtracks._need_qlen(file, tracks, "get_read_length")
            probe(f, tracks)
    while cursors:
        turn = []
        for f in list(cursors):
            contig = next(cursors[f], None) if have[f] < quota else None
            if contig is None:
                del cursors[f]
            else:
                turn.append((f, contig))
        if turn:
            for (f, contig), records in zip(turn, _bam._load_contigs([(files[f], contig) for f, contig in turn])):
                probe(f, [(contig, records)])
    return [_read_length_value(np.concatenate(t) if t else np.zeros(0, dtype=np.int32), file.name) for t, file in zip(taken, files)]


def get_read_length(bam_file: str, num_reads: int = 1000, min_mapping_quality: int = 10) -> int:
    """``get_read_length`` (rocco/scores.py:344-378): the 75th percentile of the query lengths of the first ``num_reads``
    records of ``fetch()`` that are mapped, primary and of mapping quality ``min_mapping_quality`` at least."""
    return _read_lengths([_bam._cached_file(bam_file)], num_reads, min_mapping_quality)[0]


def _mapped_reads(file) -> int:
    """pysam's ``AlignmentFile.mapped``: the index statistics summed over all contigs; for a file without an index, or
    without statistics, the ``flag & 4 == 0`` count of its decoded records."""
    from_index = getattr(file, "index_read_counts", None)
    counted = from_index() if from_index is not None else None
    if counted is not None:
        return int(counted[0])
    tracks = file.tracks()
    if isinstance(tracks, list):  # (a resident file: one launch over its contigs)
        return int(sum(_readtracks.record_flag_facts_device([records for _, records in tracks])[0])) if tracks else 0
    return int(sum(_readtracks.record_flag_facts_device([records])[0][0] for _, records in tracks))  # (decoded contig by contig)


def _contig_count(file, contig: str) -> int:
    """pysam's ``AlignmentFile.count(contig)``: the records the index iterator yields over the whole contig."""
    if contig not in file.records:
        raise ValueError(f"invalid contig `{contig}`")
    known = _known_records(file, contig)
    return int(known) if known is not None else len(file.records[contig])


def _norm_facts(files: Sequence, skip_for_norm) -> tuple:
    """rocco/scores.py:510-521: (mapped reads outside ``skip_for_norm``, `get_read_length`) of every file."""
    mapped_counts = []
    for file in files:
        mapped = _mapped_reads(file)
        for chrom in skip_for_norm:
            mapped -= _contig_count(file, chrom)
        mapped_counts.append(mapped)
    return mapped_counts, _read_lengths(files)


def get_ecdf(bam_files, length: int, chrom_sizes_file: str, nsamples=500, sample_scaling_constants: list = None, seed: int = None,
             null_stat: Callable = _null_stat, trim_proportion: float = 0.0, row_scale: float = 1000.0, pc: float = 1.0,
             files_per_call: Optional[int] = None) -> EmpiricalNull:
    """``get_ecdf`` (rocco/scores.py:642-733) over BAM paths."""
    _, files = _open_files(bam_files)
    constants = _scaling_constants(sample_scaling_constants, len(files))
    logger.info(f"Computing ECDF for representative length bin: {length} with {nsamples} samples.")
    intervals = _random_intervals(chrom_sizes_file, length=int(length), nsamples=int(nsamples), seed=seed)
    counts_t = _count_paths(files, [_null_family(intervals)], files_per_call)
    return _nulls_from_counts(counts_t, length, constants, null_stat, trim_proportion, row_scale, pc)


def multi_ecdf(bam_files, lengths, chrom_sizes_file: str, nsamples_per_length, sample_scaling_constants=None, seed=None,
               proc: int = None, null_stat: Callable = _null_stat, row_scale: float = 1000.0, pc: float = 1.0,
               files_per_call: Optional[int] = None) -> "OrderedDict":
    """``multi_ecdf`` (rocco/scores.py:741-785) over BAM paths: the regions of all lengths in one counting pass (``proc`` is
    accepted and ignored: the reference's pool runs one `get_ecdf` per length)."""
    np.random.seed(seed)
    _, files = _open_files(bam_files)
    constants = _scaling_constants(sample_scaling_constants, len(files))
    uniq_lengths, per_length = _null_intervals(lengths, chrom_sizes_file, nsamples_per_length, seed)
    for length in uniq_lengths:
        logger.info(f"Computing ECDF for representative length bin: {length} with {nsamples_per_length} samples.")
    everything = [interval for intervals in per_length for interval in intervals]
    counts_t = _count_paths(files, [_null_family(everything)], files_per_call)
    return _nulls_by_length(counts_t, uniq_lengths, per_length, constants, null_stat, row_scale, pc)


def score_peaks(bam_files, chrom_sizes_file: str = None, peak_file: str = None, count_matrix_file: str = None,
                effective_genome_size: float = None, skip_for_norm: list = _DEFAULT_SKIP_FOR_NORM, row_scale=1000, ucsc_base=250,
                threads: int = None, pc=1, ecdf_nsamples=500, ecdf_max_length_bins: int = 24, output_file="scored_peaks.bed",
                seed: int = None, proc: int = None, null_stat: Callable = _null_stat, summit_offsets_file: Optional[str] = None,
                files_per_call: Optional[int] = None):
    """``score_peaks`` (rocco/scores.py:381-639) over BAM paths; ``threads`` and ``proc`` are accepted and ignored.  The
    peaks (when ``count_matrix_file`` does not exist yet) and the random regions of every length bin are counted in ONE
    pass over the files: every contig group is decoded once and counted once, the peaks at `RAW_COUNT_OPTIONS` and the
    regions at `NULL_COUNT_OPTIONS`.  With an existing matrix file only the regions are counted.  The reference's log lines
    are emitted in its order, behind that pass.  As in the reference, the nulls always use the default statistic
    (``null_stat`` is not handed on, :552-562).  Returns (signal values, UCSC scores, p-values) and writes ``output_file``."""
    bam_files_, files = _open_files(bam_files)
    F = len(files)
    chroms, starts, ends, bed_strings, names = _read_peak_intervals(peak_file, min_columns=3)
    have_matrix = count_matrix_file is not None and os.path.exists(count_matrix_file)
    if not have_matrix and len(names) == 0:
        raise ValueError("Peak file does not contain any intervals.")
    lengths = np.asarray([end - start for start, end in zip(starts, ends)], dtype=np.float64)
    binned_lengths, ecdf_lengths = _assign_length_bins(lengths, max_bins=ecdf_max_length_bins)
    drawn = seed is None
    if drawn:
        seed = np.random.randint(1, 10000)
    np.random.seed(seed)  # (multi_ecdf, :757)
    uniq_lengths, per_length = _null_intervals(ecdf_lengths, chrom_sizes_file, ecdf_nsamples, seed)
    regions = [interval for intervals in per_length for interval in intervals]
    families = ([] if have_matrix else [_peak_family(chroms, starts, ends)]) + [_null_family(regions)]
    counts_t = _count_paths(files, families, files_per_call)
    if have_matrix:
        matrix_ = _read_count_matrix(count_matrix_file)
        null_counts_t = counts_t
    else:
        logger.info(f"Generating count matrix from {len(bam_files_)} BAM files and {peak_file} --> {count_matrix_file}")
        samples = _sample_names(bam_files_)
        _log_count_matrix_start(samples, len(names), bam_files_)
        matrix_ = counts_t[: len(names)]
        null_counts_t = counts_t[len(names):]
        if count_matrix_file is not None:
            _finish_count_matrix(count_matrix_file, samples, names, matrix_)
            matrix_ = _read_count_matrix(count_matrix_file)
        else:
            matrix_ = _reference_count_matrix(matrix_.cpu().numpy())
    mapped_counts, read_lengths = _norm_facts(files, skip_for_norm)
    constants = _scale_count_matrix(matrix_, len(names), F, chrom_sizes_file, effective_genome_size, skip_for_norm, mapped_counts,
                                    read_lengths)
    logger.info("Using %s ECDF length bins for %s unique peak lengths.", int(ecdf_lengths.size), int(np.unique(lengths).size))
    if drawn:
        logger.info(f"Using random seed: {seed} to sample length-binned regions for ECDFs.")
    for length in uniq_lengths:
        logger.info(f"Computing ECDF for representative length bin: {length} with {ecdf_nsamples} samples.")
    ecdf_dict = _nulls_by_length(null_counts_t, uniq_lengths, per_length, _scaling_constants(constants, F), _null_stat,
                                 row_scale, pc)
    for feature_idx in range(0, len(lengths), 1000):
        logger.info(f"Processing peak {feature_idx} of {len(lengths)}")
    out = _score_and_write(matrix_, lengths, binned_lengths, ecdf_dict, bed_strings, names, row_scale, pc, ucsc_base,
                           summit_offsets_file, output_file)
    logger.info(f"Scored output: {output_file}")
    return out
