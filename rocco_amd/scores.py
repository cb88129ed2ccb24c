"""Post-hoc peak scoring (rocco/scores.py).  Two halves, both on the device:

* the arithmetic after the counting (rocco/scores.py:120-149, 180-194, 560-625) -- the signal statistic, its survival
  under the empirical null of the peak's length bin, Benjamini-Hochberg q-values, the narrowPeak columns (peakscore.hip);
  the last three formatting statements (-log10, rounding to four decimals, the UCSC score) are NumPy calls on the short
  per-peak vectors, as in the reference;
* the counting itself for records already decoded (interval_count.hip): reads per peak per
  file (`raw_count_matrix_from_records`, rocco/scores.py:250-341), reads per random background region per file
  (`get_ecdf_from_records` / `multi_ecdf_from_records`, rocco/scores.py:642-785) and the composition
  (`score_peaks_from_records`, rocco/scores.py:381-639).  BAM decoding and the whole-file probes (mapped reads, read
  length) stay with the reader.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import _native
from . import dp as _dp
from . import readtracks as _readtracks


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
    # the reference's float32 per interval is min(count, 2**24); np.rint(...).astype(np.int64) of it
    count_matrix = np.minimum(counts, _readtracks.EXACT_COUNT_LIMIT).astype(np.int64)
    if output_file is not None and os.path.exists(output_file):
        os.remove(output_file)
    with open(output_file, "w", encoding="utf-8") as handle:
        handle.write("peak_name\t" + "\t".join(str(name) for name in sample_names) + "\n")
        for peak_idx, peak_name in enumerate(peak_names):
            handle.write(f"{peak_name}\t" + "\t".join(str(int(value)) for value in count_matrix[peak_idx]) + "\n")
    return output_file


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
    uniq_lengths = np.unique(lengths)
    per_length = [_random_intervals(chrom_sizes_file, length=int(length), nsamples=int(nsamples_per_length), seed=seed)
                  for length in uniq_lengths]
    everything = [interval for intervals in per_length for interval in intervals]
    counts_t = _interval_counts_device(records_by_file, [i[0] for i in everything], [i[1] for i in everything],
                                       [i[2] for i in everything], files_per_call, **NULL_COUNT_OPTIONS)
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
        matrix_ = np.minimum(counts, _readtracks.EXACT_COUNT_LIMIT).astype(np.int64)
        if count_matrix_file is not None:
            with open(count_matrix_file, "w", encoding="utf-8") as handle:
                handle.write("peak_name\t" + "\t".join(str(name) for name in sample_names) + "\n")
                for peak_idx, peak_name in enumerate(names):
                    handle.write(f"{peak_name}\t" + "\t".join(str(int(value)) for value in matrix_[peak_idx]) + "\n")
    lengths = np.asarray([end - start for start, end in zip(starts, ends)], dtype=np.float64)
    if matrix_.shape != (len(names), F):
        raise ValueError("the count matrix does not hold one row per peak and one column per file")
    if effective_genome_size is None:
        effective_genome_size = np.sum([x[1] for x in _readtracks.get_chroms_and_sizes(chrom_sizes_file).items()
                                        if x[0] not in skip_for_norm])
    mapped_sizes = np.asarray(mapped_counts, dtype=int) * np.asarray(read_lengths, dtype=int)
    sample_scaling_constants = (effective_genome_size) / mapped_sizes
    for sample_idx in range(F):
        # NumPy casts the float64 products back into the matrix's own dtype: truncation toward zero for int64 (:530-533)
        matrix_[:, sample_idx] = matrix_[:, sample_idx] * sample_scaling_constants[sample_idx]
    binned_lengths, ecdf_lengths = _assign_length_bins(lengths, max_bins=ecdf_max_length_bins)
    if seed is None:
        seed = np.random.randint(1, 10000)
    ecdf_dict = multi_ecdf_from_records(records_by_file, ecdf_lengths, chrom_sizes_file, nsamples_per_length=ecdf_nsamples,
                                        sample_scaling_constants=sample_scaling_constants, seed=seed, row_scale=row_scale, pc=pc,
                                        files_per_call=files_per_call)
    scored = score_peak_counts(matrix_.astype(np.float64), lengths, binned_lengths, ecdf_dict, row_scale=row_scale, pc=pc,
                               ucsc_base=ucsc_base)
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
    write_scored_peaks(bed_strings, names, lengths, scored, output_file, summit_offsets)
    return scored["signal"], scored["bed6_scores"], scored["pvals"]
