"""Signal-matrix assembly of rocco/readtracks.py on the MI355X.

File decoding (BAM / bigWig) stays with the reference's readers; what this module replaces is the tail of
``generate_chrom_matrix`` (rocco/readtracks.py:603-633): the union of the tracks' locus starts, the fixed-step
check for bigWig inputs and the scatter of every track's values into the dense K x m matrix -- done in HBM, so
only the per-track (start, value) lists cross PCIe and the matrix is born where the scoring kernels read it.
There is no CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import ctypes
import logging
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import dp as _dp

try:  # (optional, as in the reference: rocco/readtracks.py:17-20)
    import pyBigWig
except ImportError:  # pragma: no cover - depends on an optional package
    pyBigWig = None

logger = logging.getLogger(__name__)


def assemble_chrom_matrix_device(interval_matrix: Sequence, vals_matrix: Sequence, track_type: str = "bam",
                                 low_memory: bool = False, chromosome: str = "", device=None):
    """``interval_matrix[k]`` / ``vals_matrix[k]``: locus starts (integers) and values of track k (NumPy arrays or
    CUDA tensors).  Returns (common_intervals int64 CUDA tensor [m], matrix CUDA tensor [K, m], float64 or float32
    with ``low_memory``), as rocco/readtracks.py:614-633 does on the host."""
    import torch

    _native.load()
    if len(interval_matrix) != len(vals_matrix):
        raise ValueError("one value list per interval list is required")
    K = len(interval_matrix)
    if K == 0:
        raise ValueError("no tracks")
    dev = _dp._device(device)

    def to_dev(a, dtype):
        if _dp._is_tensor(a):
            return a.to(device=dev, dtype=dtype).contiguous().reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=dtype_np[dtype])).to(dev)

    dtype_np = {torch.int64: np.int64, torch.float64: np.float64}
    ints = [to_dev(a, torch.int64) for a in interval_matrix]
    vals = [to_dev(v, torch.float64) for v in vals_matrix]
    for a, v in zip(ints, vals):
        if a.shape[0] != v.shape[0]:
            raise ValueError("shape mismatch: value array cannot be broadcast to indexing result")  # NumPy's error
    offsets = np.zeros(K + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([int(a.shape[0]) for a in ints])
    total = int(offsets[-1])
    ints_cat = torch.cat(ints) if total else torch.empty(0, dtype=torch.int64, device=dev)
    vals_cat = torch.cat(vals) if total else torch.empty(0, dtype=torch.float64, device=dev)
    lib, solver, stream = _native.load(), _native.solver_for(dev.index), _dp._stream_ptr(ints_cat)
    common_full = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    m, fixed = ctypes.c_size_t(0), ctypes.c_int(1)
    _native.check(lib.rocco_hip_union_intervals(solver.handle, ints_cat.data_ptr(), total, common_full.data_ptr(),
                                                ctypes.byref(m), ctypes.byref(fixed), stream),
                  "rocco_hip_union_intervals")
    common = common_full[: m.value]
    if track_type == "bigwig" and m.value > 1 and not fixed.value:
        raise ValueError(f"bigWig inputs for {chromosome} do not share one fixed binning scheme")
    matrix = torch.empty((K, m.value), dtype=torch.float32 if low_memory else torch.float64, device=dev)
    off_c = (ctypes.c_size_t * (K + 1))(*[int(x) for x in offsets])
    _native.check(lib.rocco_hip_scatter_tracks(solver.handle, common.data_ptr(), m.value, ints_cat.data_ptr(),
                                               vals_cat.data_ptr(), off_c, K, 1 if low_memory else 0,
                                               matrix.data_ptr(), stream), "rocco_hip_scatter_tracks")
    return common, matrix


def assemble_chrom_matrix(interval_matrix: Sequence, vals_matrix: Sequence, track_type: str = "bam",
                          low_memory: bool = False, chromosome: str = "") -> Tuple[np.ndarray, np.ndarray]:
    """NumPy in and out: (common_intervals as ``int`` array, count_matrix), the return value of
    ``generate_chrom_matrix`` (rocco/readtracks.py:633) for tracks already decoded."""
    common_t, matrix_t = assemble_chrom_matrix_device(interval_matrix, vals_matrix, track_type=track_type,
                                                      low_memory=low_memory, chromosome=chromosome)
    return common_t.cpu().numpy().astype(int), matrix_t.cpu().numpy()


_BW_ERRORS = (
    (1, "bigWig values for {f} {c} contain non-finite entries"),
    (2, "bigWig intervals for {f} {c} contain non-positive widths"),
    (4, "bigWig file {f} uses variable-width bins on {c}; ROCCO expects a fixed-width binning scheme"),
    (8, "bigWig starts for {f} {c} are not aligned to a single fixed binning scheme"),
    (16, "bigWig file {f} has overlapping or duplicate bins on {c}"),
)


def bigwig_dense_fill_device(starts, ends, vals, const_scale: float = 1.0, round_digits: int = 5,
                             bigwig_file: str = "", chromosome: str = "", device=None):
    """What ``get_bigwig_chrom_scores`` does with a track's intervals once pyBigWig has returned them
    (rocco/readtracks.py:141-186), on the device: validation (same ValueErrors, same order), dense fill of the
    fixed-step grid between the first and the last start, constant scaling, ``np.round(..., round_digits)``.
    ``starts`` must ascend (as pyBigWig returns them).  Returns (first_start, step, values CUDA tensor)."""
    import torch

    _native.load()
    dev = _dp._device(device)

    def to_dev(a, dtype, np_dtype):
        if _dp._is_tensor(a):
            return a.to(device=dev, dtype=dtype).contiguous().reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np_dtype)).to(dev)

    starts_t, ends_t = to_dev(starts, torch.int64, np.int64), to_dev(ends, torch.int64, np.int64)
    vals_t = to_dev(vals, torch.float64, np.float64)
    count = int(starts_t.shape[0])
    if count == 0 or int(ends_t.shape[0]) != count or int(vals_t.shape[0]) != count:
        raise ValueError("starts, ends and values must be non-empty and of one length")
    lib, solver, stream = _native.load(), _native.solver_for(dev.index), _dp._stream_ptr(starts_t)
    first, step = ctypes.c_longlong(0), ctypes.c_longlong(0)
    n_full, flags = ctypes.c_size_t(0), ctypes.c_int(0)

    def call(out_t, capacity):
        _native.check(lib.rocco_hip_bigwig_dense_fill_f64(
            solver.handle, starts_t.data_ptr(), ends_t.data_ptr(), vals_t.data_ptr(), count, float(const_scale),
            int(round_digits), None if out_t is None else out_t.data_ptr(), capacity, ctypes.byref(first),
            ctypes.byref(step), ctypes.byref(n_full), ctypes.byref(flags), stream), "rocco_hip_bigwig_dense_fill_f64")
        for bit, message in _BW_ERRORS:
            if flags.value & bit:
                raise ValueError(message.format(f=bigwig_file, c=chromosome))

    call(None, 0)
    full_t = torch.empty(int(n_full.value), dtype=torch.float64, device=dev)
    call(full_t, int(n_full.value))
    return int(first.value), int(step.value), full_t


def bigwig_dense_fill(starts, ends, vals, const_scale: float = 1.0, round_digits: int = 5, bigwig_file: str = "",
                      chromosome: str = "") -> Tuple[np.ndarray, np.ndarray]:
    """NumPy in and out: the (full_intervals, rounded full_vals) pair ``get_bigwig_chrom_scores`` returns
    (rocco/readtracks.py:175-186)."""
    first, step, full_t = bigwig_dense_fill_device(starts, ends, vals, const_scale, round_digits, bigwig_file, chromosome)
    full_intervals = np.arange(first, first + step * int(full_t.shape[0]), step, dtype=np.int64)
    return full_intervals.astype(int), full_t.cpu().numpy()


# --------------------------------------------------------------------------------------------
# decoded alignment records -> binned coverage (csrc/count.hip)
# --------------------------------------------------------------------------------------------

POSITION_LIMIT = 1 << 31          # the BAM format's own limit on a position
EXACT_COUNT_LIMIT = 1 << 24       # float32 holds every integer up to here: the reference's float sums are exact below it
_RECORD_FIELDS = (("pos", np.int32), ("end", np.int32), ("isize", np.int32), ("flag", np.uint16), ("mapq", np.uint8),
                  ("mate_same", np.uint8))
_QLEN_FIELD = ("qlen", np.int32)  # the optional seventh array of `AlignmentRecords`


def _tensor_dtype(name: str, dtype) -> str:
    """The torch dtype (by name) of a record field: its own, ``flag`` as the int16 bit pattern (torch has few operators for uint16)."""
    return "int16" if name == "flag" else np.dtype(dtype).name


class CountOptions(ctypes.Structure):
    """`rocco_hip_count_options` of include/rocco_hip.h."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        "flag_include", "flag_exclude", "min_mapq", "read_length", "extend_bp", "paired_end_mode", "min_template_length",
        "max_insert_size", "shift_fwd", "shift_rev", "one_read_per_bin")]


class CountRegion(ctypes.Structure):
    """`rocco_hip_count_region` of include/rocco_hip.h."""
    _fields_ = [(name, ctypes.c_int32) for name in ("start", "end", "step", "n_bins")]


class AlignmentRecords:
    """The decoded records of one file on one chromosome, in file order (the order the index iterator yields them): six
    arrays of one length, 16 bytes per record -- ``pos`` (core.pos), ``end`` (bam_endpos), ``isize`` (core.isize) as
    int32, ``flag`` (core.flag) as uint16, ``mapq`` (core.qual) and ``mate_same`` (core.mtid == core.tid) as uint8.
    Any decoder can fill it (pysam, htslib, an integrator's own); CIGAR strings are not needed.  NumPy arrays are checked
    (integer dtypes, one length, values inside their fields, positions below 2**31) and converted; CUDA tensors must
    already have the dtypes above.

    ``qlen`` (optional, keyword or `with_query_length`): a seventh array, int32, the query length of every record --
    ``core.l_qseq``, or the CIGAR's query length (``bam_cigar2qlen``) when ``l_qseq <= 0``, the value the reference reads at
    rocco/native/ccounts_backend.c:812-816 and 1046-1050.  Only the whole-file probes read it;
    it is ``None`` unless given."""

    __slots__ = tuple(name for name, _ in _RECORD_FIELDS + (_QLEN_FIELD,))

    def __init__(self, pos, end, isize, flag, mapq, mate_same, *, qlen=None):
        given = dict(pos=pos, end=end, isize=isize, flag=flag, mapq=mapq, mate_same=mate_same, qlen=qlen)
        length = None
        for name, dtype in _RECORD_FIELDS + (_QLEN_FIELD,):
            a = given[name]
            if a is None and name == "qlen":
                self.qlen = None
                continue
            if _dp._is_tensor(a):
                kind = str(a.dtype).replace("torch.", "")
                if (kind != np.dtype(dtype).name and not (name == "flag" and kind == "int16")) or a.dim() != 1:
                    raise TypeError(f"AlignmentRecords: `{name}` must be a one-dimensional {np.dtype(dtype).name} tensor")
                a = a.contiguous()
                if kind == "uint16":
                    import torch

                    a = a.view(torch.int16)  # (the bit pattern: torch has few operators for uint16)
                if name in ("pos", "end") and a.numel() and int(a.min()) < 0:
                    raise ValueError(f"AlignmentRecords: `{name}` holds a negative position")
            else:
                a = np.asarray(a)
                if a.ndim != 1:
                    raise ValueError(f"AlignmentRecords: `{name}` must be one-dimensional")
                if a.dtype.kind == "b" and name == "mate_same":
                    a = a.astype(np.uint8)
                if a.dtype.kind not in "iu":
                    raise TypeError(f"AlignmentRecords: `{name}` must hold integers, not {a.dtype}")
                if a.size:
                    low, high = int(a.min()), int(a.max())
                    if name in ("pos", "end") and (low < 0 or high >= POSITION_LIMIT):
                        raise ValueError(f"AlignmentRecords: `{name}` must lie in [0, 2**31), the BAM format's limit on a "
                                         f"position (found {low if low < 0 else high})")
                    info = np.iinfo(dtype)
                    if low < info.min or high > info.max:
                        raise ValueError(f"AlignmentRecords: `{name}` does not fit {np.dtype(dtype).name}")
                a = np.ascontiguousarray(a, dtype=dtype)
            n = int(a.shape[0])
            if length is None:
                length = n
            elif n != length:
                raise ValueError(f"AlignmentRecords: `{name}` has {n} entries, `pos` has {length}")
            setattr(self, name, a)

    @classmethod
    def _of(cls, pos, end, isize, flag, mapq, mate_same, qlen=None) -> "AlignmentRecords":
        """Unchecked: for arrays that come from checked records or from the decoding kernel (no second pass over them)."""
        out = object.__new__(cls)
        out.pos, out.end, out.isize, out.flag, out.mapq, out.mate_same, out.qlen = pos, end, isize, flag, mapq, mate_same, qlen
        return out

    def _arrays(self) -> list:
        """The seven arrays in the order `_of` takes them (``qlen`` may be None)."""
        return [getattr(self, name) for name in self.__slots__]

    @classmethod
    def from_numpy(cls, pos, end, isize, flag, mapq, mate_same) -> "AlignmentRecords":
        return cls(pos, end, isize, flag, mapq, mate_same)

    @classmethod
    def with_query_length(cls, pos, end, isize, flag, mapq, mate_same, qlen) -> "AlignmentRecords":
        """The six arrays plus ``qlen`` (see the class): what the whole-file probes need."""
        return cls(pos, end, isize, flag, mapq, mate_same, qlen=qlen)

    def __len__(self) -> int:
        return int(self.pos.shape[0])

    def to(self, device) -> "AlignmentRecords":
        """The same records with every array on ``device``."""
        return AlignmentRecords._of(*[None if a is None else _as_tensor(name, a).to(device)
                                      for name, a in zip(self.__slots__, self._arrays())])


def _as_tensor(name: str, a):
    """A record array as a tensor where it lies (a host ``flag`` as its int16 bit pattern)."""
    import torch

    return a if _dp._is_tensor(a) else torch.from_numpy(a.view(np.int16) if name == "flag" else a)


def _compute_native_scale_factor(norm_method: str, effective_genome_size: float, step: int, mapped_reads: int,
                                 norm_read_length: int, scale_factor: float = 1.0) -> float:
    """rocco/readtracks.py:210-239: the ``norm_scale`` of a file from its whole-file facts (host arithmetic)."""
    method = "" if norm_method is None else norm_method.lower().replace(" ", "").upper()
    mapped = max(int(mapped_reads), 1)
    tile_len_kb = float(step) / 1000.0
    scale = float(scale_factor)
    if method == "RPGC":
        if effective_genome_size is None or float(effective_genome_size) <= 0:
            raise ValueError("Effective genome size must be positive for RPGC normalization.")
        current_coverage = (float(mapped) * float(max(int(norm_read_length), 1))) / float(effective_genome_size)
        return float(scale * (1.0 / max(current_coverage, 1.0e-12)))
    if method == "RPKM":
        return float(scale * (1.0 / max((float(mapped) / 1.0e6) * tile_len_kb, 1.0e-12)))
    if method in {"CPM", "BPM"}:
        return float(scale * (1.0 / max(float(mapped) / 1.0e6, 1.0e-12)))
    raise ValueError(f"Normalization method must be one of `RPGC`, `RPKM`, `CPM`, or `BPM`, not `{norm_method}`.")


def _check_exact_counts(max_magnitudes: Sequence[int]) -> None:
    """The counts equal the reference's float32 arithmetic only while every difference cell and every running value stays
    within 2**24; beyond it the reference's own result depends on the order of its records, and there is no CPU fallback."""
    for k, magnitude in enumerate(max_magnitudes):
        if int(magnitude) > EXACT_COUNT_LIMIT:
            raise RuntimeError(f"alignment counts of track {k} reach {int(magnitude)}, beyond 2**24 = {EXACT_COUNT_LIMIT}: float32 "
                               "coverage is no longer exact there (the reference's own sums depend on record order)")


def _count_options(read_length: int, one_read_per_bin=0, flag_include=0, flag_exclude=0, shift_forward_strand53=0,
                   shift_reverse_strand53=0, extend_bp=0, max_insert_size=1000, paired_end_mode=0, min_mapping_quality=0,
                   min_template_length=-1, count_mode="coverage") -> CountOptions:
    """Keyword names and defaults of the reference's ``count_alignment_region`` (rocco/_hts_counts.c:420-463)."""
    if count_mode != "coverage":
        raise ValueError(f"count mode `{count_mode}` is not built: only `coverage` (with or without one_read_per_bin)")
    return CountOptions(flag_include=int(flag_include), flag_exclude=int(flag_exclude), min_mapq=int(min_mapping_quality),
                        read_length=int(read_length), extend_bp=int(extend_bp), paired_end_mode=int(paired_end_mode),
                        min_template_length=int(min_template_length), max_insert_size=int(max_insert_size),
                        shift_fwd=int(shift_forward_strand53), shift_rev=int(shift_reverse_strand53),
                        one_read_per_bin=1 if one_read_per_bin else 0)


def _records_on_device(records_list: Sequence[AlignmentRecords], dev) -> Tuple[AlignmentRecords, list]:
    """The records of K tracks as the C ABI takes them: one `AlignmentRecords` on ``dev`` holding all of them back to back
    and the K + 1 offsets.  Every host array is uploaded once, straight to its place in the concatenated array (a device
    tensor is copied there); a single track is used where it lies."""
    import torch

    offsets = [0]
    for records in records_list:
        offsets.append(offsets[-1] + len(records))
    if len(records_list) == 1:
        return records_list[0].to(dev), offsets
    bufs = []
    for name, dtype in _RECORD_FIELDS:  # (`qlen` is not carried along: no entry point over several tracks reads it)
        bufs.append(torch.empty(offsets[-1], dtype=getattr(torch, _tensor_dtype(name, dtype)), device=dev))
        for k, records in enumerate(records_list):
            bufs[-1][offsets[k]: offsets[k + 1]].copy_(_as_tensor(name, getattr(records, name)))
    return AlignmentRecords._of(*bufs), offsets


def _record_args(records_list, cat=None, offsets=None, dev=None):
    """What every record entry point of the C ABI takes: the tracks' records back to back on one device (``cat`` and
    ``offsets`` where the caller holds them already, else uploaded to ``dev`` or to the device the tracks name), the
    T + 1 ``rec_offsets`` as ctypes reads them, and that device."""
    if cat is None:
        cat, offsets = _records_on_device(records_list, dev if dev is not None else _device_for(records_list))
    return cat, (ctypes.c_longlong * len(offsets))(*[int(o) for o in offsets]), cat.pos.device


def _records_slice(records: AlignmentRecords, lo: int, hi: int) -> AlignmentRecords:
    return AlignmentRecords._of(*[None if a is None else a[lo:hi] for a in records._arrays()])


def _count_tables(K: int, regions: Sequence, options_list: Sequence, lengths: Optional[Sequence[int]] = None):
    """The per-track arrays of the counting entry points: (options, regions, the offset of every track's counts in one
    float32 buffer -- each a multiple of four --, the length of that buffer)."""
    if K <= 0 or len(regions) != K or len(options_list) != K:
        raise ValueError("one region and one set of options per track are required")
    opts = (CountOptions * K)()
    regs = (CountRegion * K)()
    out_offsets = (ctypes.c_longlong * K)()
    total_bins = 0
    for k, (region, options) in enumerate(zip(regions, options_list)):
        start, end, step = (int(v) for v in region)
        if step <= 0 or end <= start:
            raise ValueError("invalid interval size or genomic segment")  # (the reference's wording, rocco/_hts_counts.c:500-506)
        if start < 0 or end >= POSITION_LIMIT:
            raise ValueError("a region must lie in [0, 2**31)")
        bins = ((end - start - 1) // step) + 1 if lengths is None or lengths[k] is None else int(lengths[k])
        if bins <= 0:
            raise ValueError("a track needs at least one bin")
        opts[k] = options if isinstance(options, CountOptions) else _count_options(**options)
        regs[k] = CountRegion(start, end, step, bins)
        out_offsets[k] = total_bins
        total_bins += (bins + 3) // 4 * 4
    return opts, regs, out_offsets, total_bins


def _count_concatenated(cat: AlignmentRecords, offsets: Sequence[int], regions: Sequence, options_list: Sequence,
                        lengths: Optional[Sequence[int]] = None, into=None) -> Tuple[list, list]:
    """`rocco_hip_count_alignment_records_batch` over device records already concatenated.  Returns (one float32 view per
    track, the largest magnitude the kernels saw per track: `max_magnitude_out_host`); the caller applies the 2**24 guard."""
    import torch

    lib = _native.load()
    K = len(offsets) - 1
    opts, regs, out_offsets, total_bins = _count_tables(K, regions, options_list, lengths)
    cat, rec_offsets, dev = _record_args(None, cat, offsets)
    out = torch.zeros(total_bins, dtype=torch.float32, device=dev)
    views = [out[out_offsets[k]: out_offsets[k] + regs[k].n_bins] for k in range(K)]
    if into is not None:
        for view, before in zip(views, into):
            view.copy_(before)
    maxima = (ctypes.c_longlong * K)()
    solver, stream = _native.solver_for(dev.index), _dp._stream_ptr(out)
    _native.check(lib.rocco_hip_count_alignment_records_batch(
        solver.handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.isize.data_ptr(), cat.flag.data_ptr(),
        cat.mapq.data_ptr(), cat.mate_same.data_ptr(), rec_offsets, K, ctypes.cast(opts, ctypes.c_void_p),
        ctypes.cast(regs, ctypes.c_void_p), out_offsets, 0 if into is None else 1, out.data_ptr(), maxima, stream),
        "rocco_hip_count_alignment_records_batch")
    return views, [int(m) for m in maxima]


def count_alignment_records_batch_device(records_list: Sequence[AlignmentRecords], regions: Sequence, options_list: Sequence,
                                         device=None, lengths: Optional[Sequence[int]] = None, into=None) -> list:
    """``ccounts_countRegion`` (rocco/native/ccounts_backend.c:2400-2573) for K tracks in one launch series.
    ``regions[k]``: (start, end, step); ``options_list[k]``: a `CountOptions` or a dict of `count_alignment_region`'s
    keywords plus ``read_length``.  Returns one float32 CUDA tensor per track with ((end - start - 1) // step) + 1 bins
    (``lengths[k]`` bins where given: the reference's countBufferLength).  ``into``: float32 CUDA tensors that stand for
    the reference's used count buffer: the returned tensors hold their values plus the counts (one float addition per
    bin); the tensors given are read, not changed.  Raises RuntimeError beyond 2**24."""
    K = len(records_list)
    if K == 0 or len(regions) != K or len(options_list) != K:
        raise ValueError("one region and one set of options per track are required")
    cat, offsets = _records_on_device(records_list, _dp._device(device))
    views, maxima = _count_concatenated(cat, offsets, regions, options_list, lengths, into)
    _check_exact_counts(maxima)
    return views


def count_alignment_region_from_records(records: AlignmentRecords, start: int, end: int, step: int, read_length: int,
                                        **kw) -> np.ndarray:
    """The reference's ``count_alignment_region`` (rocco/_hts_counts.c:420-569) for records already decoded: same keyword
    names and defaults (``one_read_per_bin``, ``flag_include``, ``flag_exclude``, ``shift_forward_strand53``,
    ``shift_reverse_strand53``, ``extend_bp``, ``max_insert_size=1000``, ``paired_end_mode``, ``min_mapping_quality``,
    ``min_template_length=-1``, ``count_mode="coverage"``).  Returns the float32 counts as a NumPy array."""
    kw.pop("thread_count", None)
    kw.pop("infer_fragment_length", None)
    (counts,) = count_alignment_records_batch_device([records], [(start, end, step)], [_count_options(read_length, **kw)])
    return counts.cpu().numpy()


def alignment_chrom_range_from_records(records: AlignmentRecords, chrom_size: int, flag_exclude: int = 0) -> Tuple[int, int]:
    """``ccounts_getChromRange`` (rocco/native/ccounts_backend.c:1666-1705): (pos of the first record ``flag_exclude``
    passes, end of the LAST one in file order among the records reaching into the contig's last 2 Mb); 0 where none."""
    lib = _native.load()
    dev = _device_for([records])
    r = records.to(dev)
    start, end = ctypes.c_longlong(0), ctypes.c_longlong(0)
    _native.check(lib.rocco_hip_alignment_chrom_range(
        _native.solver_for(dev.index).handle, r.pos.data_ptr(), r.end.data_ptr(), r.flag.data_ptr(), len(r), int(chrom_size),
        max(0, int(flag_exclude)) & 0xFFFF, ctypes.byref(start), ctypes.byref(end), _dp._stream_ptr(r.pos)),
        "rocco_hip_alignment_chrom_range")
    return int(start.value), int(end.value)


def _count_window(chrom_start: int, chrom_end: int, chrom_size: int, step: int) -> Tuple[int, int]:
    """rocco/readtracks.py:467-473."""
    count_start = max(0, (chrom_start // step) * step)
    count_end = min(chrom_size, int(np.ceil(max(chrom_end, count_start + 1) / float(step)) * step))
    if count_end <= count_start:
        count_end = min(chrom_size, count_start + step)
    return count_start, count_end


def _bam_tail(counts_t, count_start: int, step: int, norm_scale: float, scale_by_step: bool, const_scale: float,
              round_digits: int, bam_file: str, chromosome: str):
    """rocco/readtracks.py:492-518 on the device: scaling in float64, the positive support, np.round."""
    import torch

    lib = _native.load()
    n = int(counts_t.shape[0])
    vals_t = torch.empty(n, dtype=torch.float64, device=counts_t.device)
    first, last = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    if scale_by_step:
        logger.info(f"Dividing `vals` by step size (bp): {step}")
    if const_scale >= 0 and const_scale == 0:
        logger.warning("You are scaling the values by 0.")
    _native.check(lib.rocco_hip_alignment_count_tail_f64(
        _native.solver_for(counts_t.device.index).handle, counts_t.data_ptr(), n, float(norm_scale), 1 if scale_by_step else 0,
        float(step), float(const_scale), int(round_digits), vals_t.data_ptr(), ctypes.byref(first), ctypes.byref(last),
        _dp._stream_ptr(counts_t)), "rocco_hip_alignment_count_tail_f64")
    if first.value < 0:
        logger.warning("No non-zero values found in BAM file: %s for chromosome: %s. Returning (None,None).", bam_file, chromosome)
        return None, None
    first_idx, last_idx = int(first.value), int(last.value) + 1
    intervals = count_start + (np.arange(first_idx, last_idx, dtype=np.int64) * int(step))
    return intervals.astype(int), vals_t[first_idx:last_idx].cpu().numpy()


def bam_chrom_reads_from_records_batch(records_list: Sequence[AlignmentRecords], chrom_size: int, step: int,
                                       metadata_list: Sequence[dict], min_mapping_score: int = 10, flag_include=None,
                                       flag_exclude: int = 3844, center_reads: bool = False, const_scale: float = 1.0,
                                       round_digits: int = 5, scale_by_step: bool = False, bam_files: Optional[Sequence[str]] = None,
                                       chromosome: str = ""):
    """K files of one chromosome in one call: everything ``get_bam_chrom_reads`` does after its metadata lookup
    (rocco/readtracks.py:439-518), the counting of all files in one launch series.  Returns (interval_matrix,
    vals_matrix), the two lists `assemble_chrom_matrix` takes; a file without data has ``None`` in both (the reference's
    two ``(None, None)`` returns, with its warnings), which ``generate_chrom_matrix`` leaves out."""
    K = len(records_list)
    if len(metadata_list) != K:
        raise ValueError("one metadata dict per file is required")
    names = list(bam_files) if bam_files is not None else [""] * K
    chrom_size, step = int(chrom_size), int(step)
    intervals_out, vals_out = [None] * K, [None] * K
    if K == 0:
        return intervals_out, vals_out
    cat, offsets = _records_on_device(records_list, _device_for(records_list))
    live, regions, options = [], [], []
    for k, metadata in enumerate(metadata_list):
        chrom_start, chrom_end = alignment_chrom_range_from_records(_records_slice(cat, offsets[k], offsets[k + 1]), chrom_size,
                                                                    max(0, int(flag_exclude)))
        if chrom_end <= chrom_start:
            logger.warning("No mapped reads found in BAM file: %s for chromosome: %s. Returning (None,None).", names[k], chromosome)
            regions.append((0, 1, 1))  # (its place in the concatenated records stays; one bin nobody reads)
            options.append(_count_options(0))
            continue
        live.append(k)
        regions.append(_count_window(chrom_start, chrom_end, chrom_size, step) + (step,))
        options.append(_count_options(int(metadata["read_length"]), one_read_per_bin=1 if center_reads else 0,
                                      flag_include=max(0, int(flag_include or 0)), flag_exclude=max(0, int(flag_exclude)),
                                      extend_bp=max(0, int(metadata["resolved_extend_bp"])),
                                      paired_end_mode=1 if bool(metadata["paired_end_mode"]) else 0,
                                      min_mapping_quality=max(0, int(min_mapping_score))))
    if live:
        counts, maxima = _count_concatenated(cat, offsets, regions, options)
        _check_exact_counts([m if k in live else 0 for k, m in enumerate(maxima)])
        for k in live:
            intervals_out[k], vals_out[k] = _bam_tail(counts[k], regions[k][0], step, float(metadata_list[k]["norm_scale"]), scale_by_step,
                                                      const_scale, round_digits, names[k], chromosome)
    return intervals_out, vals_out


def bam_chrom_reads_from_records(records: AlignmentRecords, chrom_size: int, step: int, metadata: dict, min_mapping_score: int = 10,
                                 flag_include=None, flag_exclude: int = 3844, center_reads: bool = False, const_scale: float = 1.0,
                                 round_digits: int = 5, scale_by_step: bool = False, bam_file: str = "", chromosome: str = ""):
    """What ``get_bam_chrom_reads`` returns for one file (rocco/readtracks.py:439-518), from its decoded records and the
    dict of ``_get_bam_count_metadata`` (``read_length``, ``resolved_extend_bp``, ``paired_end_mode``, ``norm_scale``:
    whole-file facts; `bam_count_metadata_from_records` returns this dict from the file's decoded records, and a reader
    may as well supply it): the count window, the
    counting, the scaling and the trimming on the device.  ``(None, None)`` with the reference's warnings for an empty
    range or no positive value; otherwise ``intervals.astype(int)`` and the rounded float64 values.  This is the function
    to bind behind `get_bam_chrom_reads`."""
    intervals, vals = bam_chrom_reads_from_records_batch([records], chrom_size, step, [metadata], min_mapping_score, flag_include,
                                                         flag_exclude, center_reads, const_scale, round_digits, scale_by_step,
                                                         [bam_file], chromosome)
    return intervals[0], vals[0]


# --------------------------------------------------------------------------------------------
# K files of one chromosome -> its count matrix in one device pass (csrc/track_matrix.hip)
# --------------------------------------------------------------------------------------------

def track_matrix_shape() -> dict:
    """`rocco_hip_track_matrix_shape`: the threads of a workgroup of the fill, the elements of a row it writes at a time, the
    workgroups of one launch at most, the words of a row of its table.  No device is touched."""
    shape = (ctypes.c_int * 4)()
    _native.load().rocco_hip_track_matrix_shape(shape)
    return {"threads": int(shape[0]), "unit": int(shape[1]), "max_grid": int(shape[2]), "row_words": int(shape[3])}


def _merge_supports(grid_first, grid_last) -> Tuple[np.ndarray, np.ndarray, int]:
    """Supports ``[grid_first[k], grid_last[k]]`` (inclusive grid indices: start // step) merged into disjoint, ascending
    segments: (grid index of every segment's first bin, column of that bin, number of columns).  Supports that overlap or
    touch (``last + 1 == first``) form one segment; disjoint ones leave a gap -- the columns, laid end to end, are
    ``np.unique(np.concatenate([arange(first, last + 1) ...]))``."""
    first, last = np.asarray(grid_first, dtype=np.int64), np.asarray(grid_last, dtype=np.int64)
    if first.ndim != 1 or first.shape != last.shape or first.size == 0 or np.any(last < first):
        raise ValueError("supports must be non-empty [first, last] pairs")
    order = np.argsort(first, kind="stable")
    first, last = first[order], last[order]
    reach = np.maximum.accumulate(last)             # the furthest bin of the supports up to this one
    opens = np.ones(first.size, dtype=bool)
    opens[1:] = first[1:] > reach[:-1] + 1          # a gap in front of this support: a segment begins
    seg_first = first[opens]
    seg_last = reach[np.append(np.flatnonzero(opens)[1:] - 1, first.size - 1)]
    lengths = seg_last - seg_first + 1
    seg_col = np.zeros(seg_first.size, dtype=np.int64)
    np.cumsum(lengths[:-1], out=seg_col[1:])
    return seg_first, seg_col, int(lengths.sum())


def _segment_starts(seg_grid: np.ndarray, seg_col: np.ndarray, m: int, step: int) -> np.ndarray:
    """The locus starts of the columns of `_merge_supports`' segments (an ``int`` array, as the reference returns it)."""
    grid = np.arange(m, dtype=np.int64) + np.repeat(seg_grid - seg_col, np.diff(np.append(seg_col, m)))
    return (grid * int(step)).astype(int)


def _chrom_ranges_batch(cat: AlignmentRecords, offsets: Sequence[int], chrom_size: int, flag_exclude: int) -> list:
    """`rocco_hip_alignment_chrom_range_batch`: [(chrom_start, chrom_end)] of K tracks already concatenated, one wait."""
    K = len(offsets) - 1
    cat, rec_offsets, dev = _record_args(None, cat, offsets)
    ranges = (ctypes.c_longlong * (2 * K))()
    _native.check(_native.load().rocco_hip_alignment_chrom_range_batch(
        _native.solver_for(dev.index).handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.flag.data_ptr(), rec_offsets, K,
        int(chrom_size), max(0, int(flag_exclude)) & 0xFFFF, ranges, _dp._stream_ptr(cat.pos)), "rocco_hip_alignment_chrom_range_batch")
    return [(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(K)]


def _emit(records: Sequence[tuple]) -> None:
    """Log records collected during batched work, now, in their order: (level, message, args)."""
    for level, message, args in records:
        logger.log(level, message, *args)


def _excluded_records(names: Sequence[str], has_data: Sequence[bool], chromosome: str) -> list:
    """rocco/readtracks.py:601-613: one warning per file without data, in file order, and the last one when none has any."""
    out = [(logging.WARNING, f"No data found for {name} in chromosome {chromosome}. Excluding this track for {chromosome}.", ())
           for name, live in zip(names, has_data) if not live]
    if not any(has_data):
        out.append((logging.WARNING, f"No data found in the files {str(list(names))} for chromosome {chromosome}. Returning (None,None).", ()))
    return out


def _bam_matrix_batch(records_list, chrom_size, step, metadata_list, min_mapping_score, flag_include, flag_exclude, center_reads,
                      const_scale, round_digits, scale_by_step, low_memory, names, chromosome):
    """The work of `bam_chrom_matrix_from_records_batch` with its log records collected, not emitted: returns (starts or None,
    matrix_t or None, the records of every file in the order the reference emits them for that file, whether it has data)."""
    import torch

    K = len(records_list)
    chrom_size, step = int(chrom_size), int(step)
    file_logs = [[] for _ in range(K)]
    has_data = [False] * K
    if K == 0:
        return None, None, file_logs, has_data
    lib = _native.load()
    cat, offsets = _records_on_device(records_list, _device_for(records_list))
    ranges = _chrom_ranges_batch(cat, offsets, chrom_size, flag_exclude)  # (the first of the call's two waits)
    live, regions, options, scales = [], [], [], []
    for k, (metadata, (chrom_start, chrom_end)) in enumerate(zip(metadata_list, ranges)):
        if chrom_end <= chrom_start:
            file_logs[k].append((logging.WARNING, "No mapped reads found in BAM file: %s for chromosome: %s. Returning (None,None).",
                                 (names[k], chromosome)))
            regions.append((0, 1, 1))  # (its place in the concatenated records stays; one bin nobody reads)
            options.append(_count_options(0))
            scales.append(0.0)
            continue
        live.append(k)
        regions.append(_count_window(chrom_start, chrom_end, chrom_size, step) + (step,))
        options.append(_count_options(int(metadata["read_length"]), one_read_per_bin=1 if center_reads else 0,
                                      flag_include=max(0, int(flag_include or 0)), flag_exclude=max(0, int(flag_exclude)),
                                      extend_bp=max(0, int(metadata["resolved_extend_bp"])),
                                      paired_end_mode=1 if bool(metadata["paired_end_mode"]) else 0,
                                      min_mapping_quality=max(0, int(min_mapping_score))))
        scales.append(float(metadata["norm_scale"]))
    if not live:
        return None, None, file_logs, has_data
    opts, regs, out_offsets, total_bins = _count_tables(K, regions, options)
    cat, rec_offsets, dev = _record_args(None, cat, offsets)
    counts = torch.empty(total_bins, dtype=torch.float32, device=dev)  # (the counter writes every bin a later kernel reads)
    maxima, supports = (ctypes.c_longlong * K)(), (ctypes.c_longlong * (2 * K))()
    solver, stream = _native.solver_for(dev.index), _dp._stream_ptr(counts)
    _native.check(lib.rocco_hip_track_supports(
        solver.handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.isize.data_ptr(), cat.flag.data_ptr(), cat.mapq.data_ptr(),
        cat.mate_same.data_ptr(), rec_offsets, K, ctypes.cast(opts, ctypes.c_void_p), ctypes.cast(regs, ctypes.c_void_p), out_offsets,
        (ctypes.c_double * K)(*scales), 1 if scale_by_step else 0, float(step), float(const_scale), counts.data_ptr(), maxima,
        supports, stream), "rocco_hip_track_supports")  # (the second wait)
    _check_exact_counts([int(maxima[k]) if k in live else 0 for k in range(K)])
    rows = []
    for k in live:
        if scale_by_step:
            file_logs[k].append((logging.INFO, f"Dividing `vals` by step size (bp): {step}", ()))
        if const_scale >= 0 and const_scale == 0:
            file_logs[k].append((logging.WARNING, "You are scaling the values by 0.", ()))
        first, last = int(supports[2 * k]), int(supports[2 * k + 1])
        if first < 0:
            file_logs[k].append((logging.WARNING, "No non-zero values found in BAM file: %s for chromosome: %s. Returning (None,None).",
                                 (names[k], chromosome)))
            continue
        has_data[k] = True
        origin = regions[k][0] // step  # (count_start is a multiple of step: every track lies on one grid)
        rows.append((int(out_offsets[k]), int(regs[k].n_bins), origin, origin + first, origin + last, scales[k]))
    if not rows:
        return None, None, file_logs, has_data
    seg_grid, seg_col, m = _merge_supports([r[3] for r in rows], [r[4] for r in rows])
    words = track_matrix_shape()["row_words"]
    table = np.zeros(len(rows) * words + 2 * seg_grid.size, dtype=np.int64)
    body = table[: len(rows) * words].reshape(len(rows), words)
    body[:, :5] = np.asarray([r[:5] for r in rows], dtype=np.int64)
    body[:, 5] = np.asarray([r[5] for r in rows], dtype=np.float64).view(np.int64)
    table[len(rows) * words:] = np.stack([seg_grid, seg_col], axis=1).reshape(-1)
    table_t = torch.from_numpy(table).to(dev)  # (at most K rows and K segments go up; nothing as long as the chromosome)
    matrix = torch.empty((len(rows), m), dtype=torch.float32 if low_memory else torch.float64, device=dev)
    _native.check(lib.rocco_hip_track_matrix_fill(
        solver.handle, counts.data_ptr(), total_bins, table_t.data_ptr(), len(rows), table_t[len(rows) * words:].data_ptr(),
        int(seg_grid.size), m, 1 if scale_by_step else 0, float(step), float(const_scale), int(round_digits), 1 if low_memory else 0,
        matrix.data_ptr(), stream), "rocco_hip_track_matrix_fill")
    return _segment_starts(seg_grid, seg_col, m, step), matrix, file_logs, has_data


def bam_chrom_matrix_from_records_batch(records_list: Sequence[AlignmentRecords], chrom_size: int, step: int,
                                        metadata_list: Sequence[dict], min_mapping_score: int = 10, flag_include=None,
                                        flag_exclude: int = 3844, center_reads: bool = False, const_scale: float = 1.0,
                                        round_digits: int = 5, scale_by_step: bool = False, low_memory: bool = False,
                                        bam_files: Optional[Sequence[str]] = None, chromosome: str = ""):
    """K decoded files of one chromosome to the reference's ``(common_intervals, count_matrix)`` in one device pass: what
    ``generate_chrom_matrix`` does over BAM inputs after the metadata lookup (rocco/readtracks.py:439-518 per file, 601-633
    over the files).  The ranges of all files come from one launch, the counting and the positive supports from one launch
    series, and one kernel writes every element of the matrix once -- two waits for the device whatever K is, and neither
    the values nor the starts of a track visit the host.  Returns (starts, matrix_t): the starts as a host ``int`` array
    (built from at most K segments), the matrix as a CUDA tensor [K', m] (float64, float32 with ``low_memory``) of the K'
    files that have data, bit for bit the reference's; ``(None, None)`` when no file has data.  The reference's log records
    for the call are emitted after the batched work, in the reference's order: per file "No mapped reads...", the
    ``Dividing `vals` by step size`` line, "You are scaling the values by 0.", "No non-zero values..."; then one "No data
    found for ... Excluding..." per file without data and, when none has any, "No data found in the files ...".  RuntimeError
    beyond 2**24 (`_check_exact_counts`)."""
    K = len(records_list)
    if len(metadata_list) != K:
        raise ValueError("one metadata dict per file is required")
    names = list(bam_files) if bam_files is not None else [""] * K
    if len(names) != K:
        raise ValueError("one file name per file is required")
    starts, matrix, file_logs, has_data = _bam_matrix_batch(records_list, chrom_size, step, metadata_list, min_mapping_score,
                                                            flag_include, flag_exclude, center_reads, const_scale, round_digits,
                                                            scale_by_step, low_memory, names, chromosome)
    for records in file_logs:
        _emit(records)
    _emit(_excluded_records(names, has_data, chromosome))
    return starts, matrix


# --------------------------------------------------------------------------------------------
# decoded alignment records -> one count per (interval, file) (csrc/interval_count.hip)
# --------------------------------------------------------------------------------------------

def count_intervals_shape() -> dict:
    """`rocco_hip_count_intervals_shape`: the sizes at which the interval kernels change path."""
    shape = (ctypes.c_int * 3)()
    _native.load().rocco_hip_count_intervals_shape(shape)
    return {"unit_records": int(shape[0]), "max_grid": int(shape[1]), "waves_per_group": int(shape[2])}


def _check_intervals(chromosomes, starts, ends) -> Tuple[list, np.ndarray, np.ndarray]:
    """The argument checks of the reference's ``count_alignment_intervals`` (rocco/_hts_counts.c:571-836), its words where
    it has them."""
    chroms = [str(c) for c in chromosomes]
    starts_h, ends_h = np.asarray(starts), np.asarray(ends)
    if starts_h.ndim != 1 or ends_h.ndim != 1 or len(chroms) != starts_h.shape[0] or len(chroms) != ends_h.shape[0]:
        raise ValueError("`chromosomes`, `starts`, and `ends` must have the same length")
    if len(chroms) == 0:
        return chroms, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if starts_h.dtype.kind not in "iu" or ends_h.dtype.kind not in "iu":
        raise TypeError("starts and ends must hold integers")
    starts_h, ends_h = starts_h.astype(np.int64), ends_h.astype(np.int64)
    if np.any(ends_h <= starts_h):
        raise ValueError("each interval must satisfy end > start")
    if int(starts_h.min()) < 0 or int(ends_h.max()) >= POSITION_LIMIT:
        raise ValueError("interval positions must lie in [0, 2**31)")
    return chroms, starts_h.astype(np.int32), ends_h.astype(np.int32)


def count_alignment_intervals_batch_device(records_by_file: Sequence[dict], chroms, starts, ends, device=None, **options):
    """``count_alignment_intervals`` (rocco/_hts_counts.c:571-836: one ``ccounts_countRegion`` per interval, region =
    [start, end), one bin) for F files in one launch series.  ``records_by_file[f]``: ``{contig: AlignmentRecords}`` of file
    f, every track in coordinate order (the file order of an indexed BAM); ``chroms`` / ``starts`` / ``ends``: the P
    intervals, in any order.  ``options``: `count_alignment_region`'s keywords (``read_length`` defaults to 0; only the
    paired-end template floor reads it).  Returns the exact counts, an int32 CUDA tensor [P, F]; the reference's float is
    ``min(count, 2**24)`` (`count_alignment_intervals_from_records`)."""
    import torch

    F = len(records_by_file)
    if F == 0:
        raise ValueError("no files")
    chrom_list, starts_h, ends_h = _check_intervals(chroms, starts, ends)
    opts = _count_options(int(options.pop("read_length", 0)), **options)
    P = len(chrom_list)
    contigs = list(dict.fromkeys(chrom_list))
    for records in records_by_file:
        for contig in contigs:
            if contig not in records:
                raise ValueError("chromosome not found in alignment header")
    dev = _dp._device(device)
    if P == 0:
        return torch.zeros((0, F), dtype=torch.int32, device=dev)
    C = len(contigs)
    index = {contig: c for c, contig in enumerate(contigs)}
    ids_h = np.fromiter((index[c] for c in chrom_list), dtype=np.int32, count=P)
    tracks = [records_by_file[f][contig] for f in range(F) for contig in contigs]
    cat, rec_offsets, dev = _record_args(tracks, dev=dev)
    lib = _native.load()
    ids_t, starts_t, ends_t = (torch.from_numpy(a).to(dev) for a in (ids_h, starts_h, ends_h))
    out = torch.empty((P, F), dtype=torch.int32, device=dev)
    facts = (ctypes.c_int * (2 * F * C))()
    solver, stream = _native.solver_for(dev.index), _dp._stream_ptr(out)
    _native.check(lib.rocco_hip_count_alignment_intervals_batch(
        solver.handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.isize.data_ptr(), cat.flag.data_ptr(), cat.mapq.data_ptr(),
        cat.mate_same.data_ptr(), rec_offsets, F, C, ctypes.byref(opts), ids_t.data_ptr(), starts_t.data_ptr(), ends_t.data_ptr(),
        P, out.data_ptr(), facts, stream), "rocco_hip_count_alignment_intervals_batch")
    for t in range(F * C):
        if facts[2 * t + 1]:
            raise ValueError(f"the records of file {t // C} on {contigs[t % C]} are not in coordinate order: the interval "
                             "counter needs the file order of an indexed BAM")
    return out


COUNT_INTERVALS_MAX_SETS = 4  # ROCCO_COUNT_INTERVALS_MAX_SETS of include/rocco_hip.h


def count_alignment_intervals_sets_device(records_by_file: Sequence[dict], chroms, starts, ends, set_ids, option_sets: Sequence[dict],
                                          rows, out, col0: int = 0):
    """`count_alignment_intervals_batch_device` for a contig group that is resident once: the
    P intervals belong to ``len(option_sets)`` option sets (``set_ids[p]``; each set a dict of `count_alignment_region`'s
    keywords) and the count of interval p in file f is stored at ``out[rows[p], col0 + f]``, in one launch series with one
    wait.  ``out``: an int32 CUDA tensor [R, W] whose rows are contiguous; exactly the addressed cells are written (zeros
    included), every other cell keeps its contents.  ``rows`` must be distinct and lie in [0, R); ``col0 + F <= W``.
    Returns ``out``."""
    import torch

    F = len(records_by_file)
    if F == 0:
        raise ValueError("no files")
    chrom_list, starts_h, ends_h = _check_intervals(chroms, starts, ends)
    P, S = len(chrom_list), len(option_sets)
    if not 1 <= S <= COUNT_INTERVALS_MAX_SETS:
        raise ValueError(f"between 1 and {COUNT_INTERVALS_MAX_SETS} option sets are required")
    opts = (CountOptions * S)(*[_count_options(int(o.get("read_length", 0)), **{k: v for k, v in o.items() if k != "read_length"})
                                for o in option_sets])
    sets_h, rows_h = np.asarray(set_ids), np.asarray(rows)
    if sets_h.shape != (P,) or rows_h.shape != (P,):
        raise ValueError("one set id and one row per interval are required")
    if not _dp._is_tensor(out) or not out.is_cuda or out.dtype != torch.int32 or out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1):
        raise TypeError("`out` must be a two-dimensional int32 CUDA tensor with contiguous rows")
    col0 = int(col0)
    if col0 < 0 or col0 + F > int(out.shape[1]):
        raise ValueError("`col0` and the files do not fit into a row of `out`")
    if P == 0:
        return out
    if sets_h.dtype.kind not in "iu" or rows_h.dtype.kind not in "iu":
        raise TypeError("set ids and rows must hold integers")
    if int(sets_h.min()) < 0 or int(sets_h.max()) >= S:
        raise ValueError("a set id names no option set")
    if int(rows_h.min()) < 0 or int(rows_h.max()) >= int(out.shape[0]):
        raise ValueError("a row lies outside `out`")
    if np.unique(rows_h).size != P:
        raise ValueError("the rows of one call must be distinct")
    contigs = list(dict.fromkeys(chrom_list))
    for records in records_by_file:
        for contig in contigs:
            if contig not in records:
                raise ValueError("chromosome not found in alignment header")
    dev = out.device
    C = len(contigs)
    index = {contig: c for c, contig in enumerate(contigs)}
    ids_h = np.fromiter((index[c] for c in chrom_list), dtype=np.int32, count=P)
    cat, rec_offsets, dev = _record_args([records_by_file[f][contig] for f in range(F) for contig in contigs], dev=dev)
    ids_t, starts_t, ends_t, sets_t, rows_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
        ids_h, starts_h, ends_h, sets_h.astype(np.int32), rows_h.astype(np.int64)))
    facts = (ctypes.c_int * (2 * F * C))()
    solver, stream = _native.solver_for(dev.index), _dp._stream_ptr(out)
    _native.check(_native.load().rocco_hip_count_alignment_intervals_sets(
        solver.handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.isize.data_ptr(), cat.flag.data_ptr(), cat.mapq.data_ptr(),
        cat.mate_same.data_ptr(), rec_offsets, F, C, ctypes.cast(opts, ctypes.c_void_p), S, sets_t.data_ptr(), ids_t.data_ptr(),
        starts_t.data_ptr(), ends_t.data_ptr(), rows_t.data_ptr(), P, out.data_ptr(), int(out.shape[0]),
        int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1]), col0, facts, stream), "rocco_hip_count_alignment_intervals_sets")
    for t in range(F * C):
        if facts[2 * t + 1]:
            raise ValueError(f"the records of file {col0 + t // C} on {contigs[t % C]} are not in coordinate order: the interval "
                             "counter needs the file order of an indexed BAM")
    return out


def count_alignment_intervals_from_records(records_by_chrom: dict, chromosomes, starts, ends, **kw) -> np.ndarray:
    """The reference's ``count_alignment_intervals`` (rocco/_hts_counts.c:571-836) for one file's decoded records
    (``{contig: AlignmentRecords}``): same keyword names and defaults as `count_alignment_region_from_records`
    (``thread_count`` and ``infer_fragment_length`` are accepted and ignored).  Returns float32 counts, one per interval,
    clamped at 2**24: the reference adds 1.0f into one float, and float32(2**24) + 1 rounds back to 2**24 (derived from
    float32 arithmetic, not recorded from the reference at that depth)."""
    kw.pop("thread_count", None)
    kw.pop("infer_fragment_length", None)
    counts = count_alignment_intervals_batch_device([records_by_chrom], chromosomes, starts, ends, **kw)
    return np.minimum(counts[:, 0].cpu().numpy(), EXACT_COUNT_LIMIT).astype(np.float32)


# --------------------------------------------------------------------------------------------
# decoded records of a whole file -> the count metadata (csrc/fragment_length.hip)
# --------------------------------------------------------------------------------------------

class AlignmentFileRecords:
    """The decoded records of one whole file: ``contigs``, the header's ``(name, length)`` pairs IN HEADER ORDER, and
    ``records``, a mapping from contig name to `AlignmentRecords` in file order (absent or empty contigs allowed).
    Concatenating the contigs in header order is the file order of a coordinate-sorted, indexed BAM, which the probes
    that read "the first N records of the file" rely on.  Records without a contig (tid -1) are not part of it; they lie
    at the end of such a file, so a result can differ from the reference's only for a file with fewer placed records than a
    probe looks at (4 096 at the defaults).  ``name`` is the file's name in messages.  A ``(contigs, records)`` pair is
    accepted wherever one of these is."""

    __slots__ = ("contigs", "records", "name")

    def __init__(self, contigs, records, name: str = ""):
        self.contigs = [(str(n), int(length)) for n, length in contigs]
        if len({n for n, _ in self.contigs}) != len(self.contigs):
            raise ValueError("AlignmentFileRecords: a contig is named twice")
        known = {n for n, _ in self.contigs}
        for contig in records:
            if contig not in known:
                raise ValueError(f"AlignmentFileRecords: records for `{contig}`, which the header does not name")
        self.records = dict(records)
        self.name = str(name)

    def tracks(self, names=None) -> list:
        """(contig, records) in header order (or for ``names`` in their order), contigs without records left out."""
        order = [n for n, _ in self.contigs] if names is None else list(names)
        return [(n, self.records[n]) for n in order if n in self.records and len(self.records[n]) > 0]


def _as_file(file) -> AlignmentFileRecords:
    if isinstance(file, AlignmentFileRecords):
        return file
    contigs, records = file
    return AlignmentFileRecords(contigs, records)


def _need_qlen(file: AlignmentFileRecords, tracks, what: str) -> None:
    if getattr(tracks, "carries_qlen", False):  # (lazy tracks of an indexed file: decoded as a probe reaches them, always with `qlen`)
        return
    for contig, records in tracks:
        if records.qlen is None:
            raise ValueError(f"{what}: the records of {file.name or 'the file'} on {contig} carry no `qlen` (query length); build "
                             "them with AlignmentRecords.with_query_length")


def _host(a) -> np.ndarray:
    if _dp._is_tensor(a):
        a = a.cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a
    return a


def _head_chunks(tracks, fields, first: int = 4096):
    """The records of ``tracks`` in order, as host arrays of ``fields``, a head slice at a time (doubling): the probes that
    look at the head of a file download what they look at, not whole arrays."""
    size = max(int(first), 1)
    for _, records in tracks:
        n, at = len(records), 0
        while at < n:
            hi = min(n, at + size)
            yield {f: _host(getattr(records, f)[at:hi]) for f in fields}
            at, size = hi, size * 2


def _uint_median(values: np.ndarray) -> int:
    """The integer median of the reference's probes (e.g. rocco/native/ccounts_backend.c:830-845): sort, the middle one, or
    (a + b) / 2 in unsigned arithmetic."""
    v = np.sort(np.asarray(values, dtype=np.int64))
    mid = v.size // 2
    return int((v[mid - 1] + v[mid]) // 2) if v.size % 2 == 0 else int(v[mid])


def is_alignment_paired_end_from_records(file, max_reads: int = 1000) -> bool:
    """``ccounts_isPairedEnd`` (rocco/native/ccounts_backend.c:598-652) for a file's decoded records: whether one of the
    first ``max_reads`` records in file order is paired (every record for ``max_reads <= 0``).  Host arithmetic on a
    downloaded head."""
    file = _as_file(file)
    left = int(max_reads)
    for chunk in _head_chunks(file.tracks(), ("flag",), first=left if left > 0 else 1 << 16):
        flags = chunk["flag"] if left <= 0 else chunk["flag"][:left]
        if np.any(flags & 1):
            return True
        if left > 0:
            left -= flags.size
            if left <= 0:
                return False
    return False


def alignment_read_length_from_records(file, min_reads: int = 32, max_iterations: int = 4096, flag_exclude: int = 0) -> int:
    """``ccounts_getReadLength`` (rocco/native/ccounts_backend.c:654-856, the alignment branch) for a file's decoded
    records: of the first ``max_iterations`` records in file order, the first ``min_reads`` with ``qlen > 0`` that pass
    ``flag_exclude``; their integer median.  RuntimeError with the reference's message when none qualifies.  Host arithmetic
    on a downloaded head."""
    file = _as_file(file)
    tracks = file.tracks()
    _need_qlen(file, tracks, "alignment_read_length_from_records")
    min_reads = max(int(min_reads), 1)
    left = max(int(max_iterations), min_reads)
    exclude = int(flag_exclude) & 0xFFFF
    taken, have = [], 0
    for chunk in _head_chunks(tracks, ("flag", "qlen"), first=left):
        flags, qlen = chunk["flag"][:left], chunk["qlen"][:left]
        good = qlen[((flags & exclude) == 0) & (qlen > 0)][: min_reads - have]
        taken.append(good)
        have += good.size
        left -= flags.size
        if have >= min_reads or left <= 0:
            break
    if have == 0:
        raise RuntimeError("failed to estimate read length")
    return _uint_median(np.concatenate(taken))


def _device_for(tracks):
    """The device the first track on a device names, else the current one."""
    given = next((r.pos.device for r in tracks if _dp._is_tensor(r.pos)), None)
    return given if given is not None else _dp._device()


def record_flag_facts_device(records_list: Sequence[AlignmentRecords], cat=None, offsets=None) -> Tuple[list, list]:
    """`rocco_hip_record_flag_facts`: per track the number of records with ``flag & 4 == 0`` and whether its ``pos`` fails to
    ascend."""
    T = len(records_list)
    if T == 0:
        return [], []
    lib = _native.load()
    cat, rec_offsets, dev = _record_args(records_list, cat, offsets)
    mapped, unsorted = (ctypes.c_longlong * T)(), (ctypes.c_int * T)()
    _native.check(lib.rocco_hip_record_flag_facts(_native.solver_for(dev.index).handle, cat.pos.data_ptr(), cat.flag.data_ptr(), rec_offsets,
                                                  T, mapped, unsorted, _dp._stream_ptr(cat.pos)), "rocco_hip_record_flag_facts")
    return [int(m) for m in mapped], [int(u) for u in unsorted]


def alignment_mapped_read_count_from_records(file, exclude_chromosomes=()) -> Tuple[int, int]:
    """``ccounts_getMappedReadCount`` (rocco/native/ccounts_backend.c:1712-1888, the alignment branch) for a file's decoded
    records: (mapped, unmapped) summed over the contigs not in ``exclude_chromosomes``, as the index statistics count them
    (``flag & 4``).  The unmapped count leaves out the records without a contig, which are not part of the input (the
    reference's callers drop it)."""
    file = _as_file(file)
    excluded = {str(c) for c in (exclude_chromosomes or ())}
    from_index = getattr(file, "index_read_counts", None)  # (an indexed file: the index statistics, as the reference reads them)
    counted = from_index(excluded) if from_index is not None else None
    if counted is not None:
        return counted
    tracks = [(n, r) for n, r in file.tracks() if n not in excluded]
    if not tracks:
        return 0, 0
    mapped, _ = record_flag_facts_device([r for _, r in tracks])
    total = sum(len(r) for _, r in tracks)
    return int(sum(mapped)), int(total - sum(mapped))


def fragment_length_shape() -> dict:
    """`rocco_hip_fragment_length_shape`: the sizes the fragment-length kernels are built to."""
    shape = (ctypes.c_int * 4)()
    _native.load().rocco_hip_fragment_length_shape(shape)
    return {"threads": int(shape[0]), "density_records": int(shape[1]), "density_window": int(shape[2]), "max_block_size": int(shape[3])}


def _fragment_params(flag_exclude, max_iterations, max_insert_size, block_size, rolling_chunk_size, lag_step, early_exit, fallback) -> dict:
    """rocco/native/ccounts_backend.c:940-967."""
    p = dict(flag_exclude=int(flag_exclude) & 0xFFFF if int(flag_exclude) > 0 else 0, max_iterations=max(int(max_iterations), 1),
             max_insert_size=max(int(max_insert_size), 1), block_size=max(int(block_size), 64),
             rolling_chunk_size=max(int(rolling_chunk_size), 1), lag_step=max(int(lag_step), 1), early_exit=int(early_exit),
             fallback=int(fallback) if int(fallback) > 0 else 0)
    if p["early_exit"] < 1:
        p["early_exit"] = p["max_iterations"]
    return p


def _top_contigs(contigs) -> list:
    """rocco/native/ccounts_backend.c:994-1013: the three longest contigs; a strictly longer one replaces, so the first of
    equals stays ahead; a length of 0 never enters."""
    top = []
    for name, length in contigs:
        for i in range(3):
            if i >= len(top) or length > top[i][1]:
                if length > 0:
                    top.insert(i, (name, length))
                    del top[3:]
                break
    return top


def _sample_pass(tracks, flag_exclude: int, max_iterations: int) -> Tuple[int, float, bool]:
    """rocco/native/ccounts_backend.c:1015-1060 on a downloaded head: (records sampled, the sum of their query lengths,
    whether a record seen up to the last sampled one -- passing the flags, mapped, of any query length -- is paired)."""
    count, total, paired = 0, 0.0, False
    for chunk in _head_chunks(tracks, ("flag", "qlen"), first=max(4096, 2 * max_iterations)):
        flags, qlen = chunk["flag"].astype(np.int64), chunk["qlen"]
        seen = ((flags & flag_exclude) == 0) & ((flags & 4) == 0)
        sampled = seen & (qlen > 0)
        running = np.cumsum(sampled)
        need = max_iterations - count
        if running.size and running[-1] >= need:
            last = int(np.searchsorted(running, need))  # the record that completes the sample
            seen, sampled = seen[: last + 1], sampled[: last + 1]
            flags, qlen = flags[: last + 1], qlen[: last + 1]
        count += int(sampled.sum())
        total += float(qlen[sampled].astype(np.int64).sum())  # (integers: exact in a double, as the reference's running sum)
        paired = paired or bool(np.any(seen & ((flags & 1) != 0)))
        if count >= max_iterations:
            break
    return count, total, paired


def fragment_block_centers_device(records_list: Sequence[AlignmentRecords], contig_lengths: Sequence[int], flag_exclude: int = 0,
                                  max_iterations: int = 1000, block_size: int = 5000, rolling_chunk_size: int = 250,
                                  return_density: bool = False, cat=None, offsets=None):
    """`rocco_hip_fragment_block_centers` (rocco/native/ccounts_backend.c:1217-1339) per track: the block centres (chunk
    indices) in the order the reference accepts them, as a list of int32 arrays.  With ``return_density`` also the window
    sums and the ranking per track (int32 CUDA tensors)."""
    import torch

    T = len(records_list)
    lib = _native.load()
    cat, rec_offsets, dev = _record_args(records_list, cat, offsets)
    lengths = (ctypes.c_longlong * T)(*[int(n) for n in contig_lengths])
    chunks = [0 if int(n) < block_size else max((int(n) + rolling_chunk_size - 1) // rolling_chunk_size, 0) for n in contig_lengths]
    chunk_offsets = (ctypes.c_longlong * (T + 1))(*np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64).tolist())
    density = rank = None
    if return_density:
        density = torch.empty(max(int(chunk_offsets[T]), 1), dtype=torch.int32, device=dev)
        rank = torch.empty_like(density)
    centers, counts = (ctypes.c_int * (T * int(max_iterations)))(), (ctypes.c_int * T)()
    _native.check(lib.rocco_hip_fragment_block_centers(
        _native.solver_for(dev.index).handle, cat.pos.data_ptr(), cat.flag.data_ptr(), rec_offsets, T, lengths, int(flag_exclude),
        int(max_iterations), int(block_size), int(rolling_chunk_size), centers, counts, chunk_offsets,
        None if density is None else density.data_ptr(), None if rank is None else rank.data_ptr(), _dp._stream_ptr(cat.pos)),
        "rocco_hip_fragment_block_centers")
    flat = np.ctypeslib.as_array(centers)
    picked = [flat[t * int(max_iterations): t * int(max_iterations) + int(counts[t])].copy() for t in range(T)]
    if not return_density:
        return picked
    return (picked, [density[chunk_offsets[t]: chunk_offsets[t + 1]] for t in range(T)],
            [rank[chunk_offsets[t]: chunk_offsets[t + 1]] for t in range(T)])


def _block_starts(centers: np.ndarray, contig_length: int, block_size: int, rolling_chunk_size: int) -> np.ndarray:
    """rocco/native/ccounts_backend.c:1343-1359 (the contig is at least a block long, so the clamped start is never negative)."""
    starts = centers.astype(np.int64) * rolling_chunk_size + (rolling_chunk_size // 2) - (block_size // 2)
    starts = np.maximum(starts, 0)
    return np.where(starts + block_size > contig_length, contig_length - block_size, starts)


def strand_xcorr_blocks_device(records_list: Sequence[AlignmentRecords], block_track, block_start, min_lag, flag_exclude: int = 0,
                               block_size: int = 5000, max_insert_size: int = 1000, lag_step: int = 5, cat=None, offsets=None):
    """`rocco_hip_strand_xcorr_blocks` (rocco/native/ccounts_backend.c:1361-1469): for block b = [block_start[b], +block_size)
    of track block_track[b], (best_lag int32, best_score float64, fwd_sum int32, rev_sum int32) as NumPy arrays; ``min_lag``
    per track.  A block is a candidate iff ``best_lag > 0 and best_score != 0.0``.  ``pos`` must ascend in every track."""
    limit = fragment_length_shape()["max_block_size"]
    if int(block_size) > limit:
        raise ValueError(f"block_size {int(block_size)} is beyond {limit}: the two strand arrays of a block must fit one workgroup's "
                         "LDS (there is no CPU fallback)")
    T, B = len(records_list), len(block_track)
    lib = _native.load()
    cat, rec_offsets, dev = _record_args(records_list, cat, offsets)
    tracks = (ctypes.c_int * B)(*[int(t) for t in block_track])
    starts = (ctypes.c_longlong * B)(*[int(s) for s in block_start])
    lags = (ctypes.c_int * T)(*[int(v) for v in min_lag])
    best_lag, fwd_sum, rev_sum, best_score = (ctypes.c_int * B)(), (ctypes.c_int * B)(), (ctypes.c_int * B)(), (ctypes.c_double * B)()
    _native.check(lib.rocco_hip_strand_xcorr_blocks(
        _native.solver_for(dev.index).handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.flag.data_ptr(), rec_offsets, T, tracks, starts, B,
        lags, int(flag_exclude), int(block_size), int(max_insert_size), int(lag_step), best_lag, best_score, fwd_sum, rev_sum,
        _dp._stream_ptr(cat.pos)), "rocco_hip_strand_xcorr_blocks")
    return (np.ctypeslib.as_array(best_lag).copy(), np.ctypeslib.as_array(best_score).copy(), np.ctypeslib.as_array(fwd_sum).copy(),
            np.ctypeslib.as_array(rev_sum).copy())


def _clamped_median(values, low: int, high: int) -> int:
    """rocco/native/ccounts_backend.c:1149-1168 and 1485-1504."""
    return min(max(_uint_median(values), low), high)


def _paired_fragment_lengths(jobs: list, p: dict) -> None:
    """rocco/native/ccounts_backend.c:1084-1180 for every paired file of ``jobs``: predicate and compaction on the device,
    the first max(max_iterations, 2000) lengths in contig order, their median."""
    import torch

    lib = _native.load()
    tracks = [(j, r) for j in jobs for _, r in j["tracks"]]
    if not tracks:
        return
    records = [r for _, r in tracks]
    cat, rec_offsets, dev = _record_args(records)
    offsets, T = list(rec_offsets), len(tracks)
    total = max(int(offsets[-1]), 1)
    tmp, out = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    floors = (ctypes.c_int * T)(*[int(j["min_insert"]) for j, _ in tracks])
    counts = (ctypes.c_longlong * T)()
    _native.check(lib.rocco_hip_template_lengths(
        _native.solver_for(dev.index).handle, cat.isize.data_ptr(), cat.flag.data_ptr(), cat.mate_same.data_ptr(), rec_offsets, T, floors,
        p["flag_exclude"], p["max_insert_size"], tmp.data_ptr(), out.data_ptr(), counts, _dp._stream_ptr(cat.pos)),
        "rocco_hip_template_lengths")
    required = max(p["max_iterations"], 2000)
    taken = {id(j): [] for j in jobs}
    for t, (job, _) in enumerate(tracks):
        have = sum(a.size for a in taken[id(job)])
        take = min(int(counts[t]), required - have)
        if take > 0:
            taken[id(job)].append(out[offsets[t]: offsets[t] + take].cpu().numpy())
    for job in jobs:
        if taken[id(job)]:
            job["result"] = _clamped_median(np.concatenate(taken[id(job)]), job["min_insert"], p["max_insert_size"])


def _single_end_fragment_lengths(jobs: list, p: dict) -> None:
    """rocco/native/ccounts_backend.c:1182-1509 for every single-end file of ``jobs``: block centres of all their contigs in
    one call, then the blocks of all files in rounds -- each file submits the next blocks of the contig it is in, in the
    reference's order, and stops where the reference stops (``early_exit`` candidates, moving to its next contig only while
    fewer exist); surplus blocks of a round are discarded."""
    block_size, chunk = p["block_size"], p["rolling_chunk_size"]
    limit = fragment_length_shape()["max_block_size"]
    if block_size > limit:
        raise ValueError(f"block_size {block_size} is beyond {limit}: the two strand arrays of a block must fit one workgroup's LDS "
                         "(there is no CPU fallback)")
    tracks = [(j, contig, length, r) for j in jobs for (contig, r), length in zip(j["tracks"], j["track_lengths"])]
    if not tracks:
        return
    records = [r for _, _, _, r in tracks]
    cat, offsets = _records_on_device(records, _device_for(records))
    _, unsorted = record_flag_facts_device(records, cat, offsets)
    for (job, contig, _, _), bad in zip(tracks, unsorted):
        if bad:
            raise ValueError(f"the records of file {job['name']} on {contig} are not in coordinate order: the fragment-length "
                             "estimate needs the file order of an indexed BAM")
    centers = fragment_block_centers_device(records, [length for _, _, length, _ in tracks], p["flag_exclude"], p["max_iterations"],
                                            block_size, chunk, cat=cat, offsets=offsets)
    min_lag = [int(j["min_insert"]) for j, _, _, _ in tracks]
    for t, (job, _, length, _) in enumerate(tracks):
        job.setdefault("queue", []).append((t, _block_starts(centers[t], length, block_size, chunk)))
        job.update(at=0, lags=[])
    live = [j for j in jobs if j.get("queue")]
    while live:
        block_track, block_start, owners = [], [], []
        for job in live:
            t, starts = job["queue"][0]
            n = min(starts.size - job["at"], max(64, 2 * (p["early_exit"] - len(job["lags"]))))
            block_track += [t] * n
            block_start += starts[job["at"]: job["at"] + n].tolist()
            owners.append((job, n))
        if block_track:
            best_lag, best_score, _, _ = strand_xcorr_blocks_device(records, block_track, block_start, min_lag, p["flag_exclude"], block_size,
                                                                     p["max_insert_size"], p["lag_step"], cat=cat, offsets=offsets)
        at = 0
        for job, n in owners:
            for b in range(at, at + n):
                if len(job["lags"]) >= p["early_exit"]:
                    break
                if best_lag[b] > 0 and best_score[b] != 0.0:
                    job["lags"].append(int(best_lag[b]) + 1)
            at += n
            job["at"] += n
            if job["at"] >= job["queue"][0][1].size:
                job["queue"].pop(0)
                job["at"] = 0
            if len(job["lags"]) >= p["early_exit"]:
                job["queue"] = []
        live = [j for j in live if j["queue"]]
    for job in jobs:
        if job.get("lags"):
            job["result"] = _clamped_median(job["lags"], job["min_insert"], p["max_insert_size"])


def alignment_fragment_length_from_records_batch(files: Sequence, flag_exclude: int = 0, max_iterations: int = 1000,
                                                 max_insert_size: int = 1000, block_size: int = 5000, rolling_chunk_size: int = 250,
                                                 lag_step: int = 5, early_exit: int = 250, fallback: int = 0) -> list:
    """``ccounts_getFragmentLength`` (rocco/native/ccounts_backend.c:861-1524; keywords and defaults of
    ``get_alignment_fragment_length``, rocco/_hts_counts.c:196-205) for F files' decoded records in one launch series: per
    file the fragment length (paired-end: the median template length; single-end: the median of the best strand
    cross-correlation lags + 1 over its densest blocks), ``fallback`` where nothing qualifies (0 for ``fallback <= 0``).
    The records need ``qlen``; every contig's ``pos`` must ascend (ValueError naming file and contig otherwise).  The
    sample pass runs on a downloaded head; density, ranking, cross-correlation and the paired branch's compaction run on
    the device; a ``block_size`` beyond `fragment_length_shape`'s limit is a ValueError."""
    p = _fragment_params(flag_exclude, max_iterations, max_insert_size, block_size, rolling_chunk_size, lag_step, early_exit, fallback)
    jobs, paired_jobs, single_jobs = [], [], []
    for k, given in enumerate(files):
        file = _as_file(given)
        top = _top_contigs(file.contigs)
        tracks = file.tracks([n for n, _ in top])
        _need_qlen(file, tracks, "alignment_fragment_length_from_records")
        lengths = dict(top)
        job = {"name": file.name or str(k), "tracks": tracks, "track_lengths": [lengths[n] for n, _ in tracks], "result": p["fallback"]}
        jobs.append(job)
        count, total, paired = _sample_pass(tracks, p["flag_exclude"], p["max_iterations"])
        if count <= 0:
            continue
        job["min_insert"] = min(max(int(total / float(count)), 1), p["max_insert_size"])
        (paired_jobs if paired else single_jobs).append(job)
    if paired_jobs:
        _paired_fragment_lengths(paired_jobs, p)
    if single_jobs:
        _single_end_fragment_lengths(single_jobs, p)
    return [int(job["result"]) for job in jobs]


def alignment_fragment_length_from_records(file, flag_exclude: int = 0, max_iterations: int = 1000, max_insert_size: int = 1000,
                                           block_size: int = 5000, rolling_chunk_size: int = 250, lag_step: int = 5, early_exit: int = 250,
                                           fallback: int = 0) -> int:
    """One file of `alignment_fragment_length_from_records_batch`."""
    return alignment_fragment_length_from_records_batch([file], flag_exclude, max_iterations, max_insert_size, block_size,
                                                        rolling_chunk_size, lag_step, early_exit, fallback)[0]


def bam_count_metadata_from_records_batch(files: Sequence, step: int, norm_method: str, effective_genome_size: float, ignore_for_norm,
                                          flag_exclude: int = 0, extend_reads: int = -1, scale_factor: float = 1.0,
                                          bam_files: Optional[Sequence[str]] = None) -> list:
    """`bam_count_metadata_from_records` for K files: the fragment lengths of all files that need one (``extend_reads == 0``)
    come from one launch series."""
    files = [_as_file(f) for f in files]
    names = list(bam_files) if bam_files is not None else [f.name for f in files]
    ignore = tuple(ignore_for_norm or [])
    facts = []
    for file in files:
        paired_end = bool(is_alignment_paired_end_from_records(file, max_reads=1024))
        read_length = int(alignment_read_length_from_records(file, min_reads=32, max_iterations=4096, flag_exclude=max(0, int(flag_exclude))))
        mapped_reads, _ = alignment_mapped_read_count_from_records(file, exclude_chromosomes=list(ignore))
        facts.append((paired_end, read_length, mapped_reads))
    fragment_lengths = [None] * len(files)
    if int(extend_reads) == 0:  # `_estimate_fragment_length` (rocco/readtracks.py:189-207)
        lengths = alignment_fragment_length_from_records_batch(files, flag_exclude=max(0, int(flag_exclude)), max_iterations=4096, fallback=0)
        fragment_lengths = [n if n > 0 else None for n in lengths]
    out = []
    for bam_file, (paired_end, read_length, mapped_reads), fragment_length in zip(names, facts, fragment_lengths):
        norm_read_length, resolved_extend_bp, paired_end_mode = int(read_length), int(extend_reads), False
        if int(extend_reads) == 0:
            if paired_end:
                if fragment_length is not None and fragment_length > 0:
                    norm_read_length, paired_end_mode, resolved_extend_bp = int(fragment_length), True, 0
                else:
                    logger.warning("Could not estimate fragment length for %s; falling back to read length %s.", bam_file, read_length)
            else:
                if fragment_length is not None and fragment_length > int(read_length):
                    norm_read_length = resolved_extend_bp = int(fragment_length)
                    logger.info("Using inferred single-end fragment length %s for %s.", fragment_length, bam_file)
                else:
                    logger.warning("`extend_reads=0` requests fragment-length inference, but %s did not yield a larger single-end "
                                   "fragment length; using read length %s.", bam_file, read_length)
                    resolved_extend_bp = -1
        elif int(extend_reads) > 0:
            norm_read_length = resolved_extend_bp = int(extend_reads)
        norm_scale = _compute_native_scale_factor(norm_method=norm_method, effective_genome_size=effective_genome_size, step=step,
                                                  mapped_reads=int(mapped_reads), norm_read_length=int(norm_read_length),
                                                  scale_factor=float(scale_factor))
        out.append({"paired_end": paired_end, "paired_end_mode": paired_end_mode, "read_length": int(read_length),
                    "norm_read_length": int(norm_read_length), "resolved_extend_bp": int(resolved_extend_bp),
                    "mapped_reads": int(mapped_reads), "norm_scale": float(norm_scale)})
    return out


def bam_count_metadata_from_records(file, step: int, norm_method: str, effective_genome_size: float, ignore_for_norm,
                                    flag_exclude: int = 0, extend_reads: int = -1, scale_factor: float = 1.0, bam_file: str = "") -> dict:
    """The body of the reference's ``_get_bam_count_metadata`` after its cache lookup (rocco/readtracks.py:269-351) for a
    file's decoded records (`AlignmentFileRecords`, with ``qlen``): the four probes above, the same ``extend_reads``
    branches, the same three log lines at the same levels, `_compute_native_scale_factor` as it is.  Returns the
    reference's dict without ``threads`` (host configuration, like its cache): ``paired_end``, ``paired_end_mode``,
    ``read_length``, ``norm_read_length``, ``resolved_extend_bp``, ``mapped_reads``, ``norm_scale`` -- the ``metadata`` that
    `bam_chrom_reads_from_records` takes.  This is the function to bind behind `_get_bam_count_metadata`."""
    file = _as_file(file)
    return bam_count_metadata_from_records_batch([file], step, norm_method, effective_genome_size, ignore_for_norm, flag_exclude,
                                                 extend_reads, scale_factor, [bam_file or file.name])[0]


# --------------------------------------------------------------------------------------------
# the reference's two entry points around the kernels above (same names, arguments, return values and errors)
# --------------------------------------------------------------------------------------------

def _require_pybigwig():
    """rocco/readtracks.py:75-80."""
    if pyBigWig is None:
        raise ImportError("bigWig input requires the optional `pyBigWig` dependency...try `python -m pip install pybigwig`")
    return pyBigWig


def _get_track_type(track_file: str) -> str:
    """rocco/readtracks.py:83-91."""
    ext = os.path.splitext(track_file)[1].lower().lstrip(".")
    if ext == "bam":
        return "bam"
    if ext in {"bw", "bigwig"}:
        return "bigwig"
    raise ValueError(f"Unsupported input file type for `{track_file}`. Expected BAM or bigWig.")


def get_chroms_and_sizes(chrom_sizes_file) -> dict:
    """rocco/readtracks.py:362-386: ``{chromosome: size}`` from a two-column tab-separated file."""
    if chrom_sizes_file is None or not os.path.exists(chrom_sizes_file):
        raise FileNotFoundError(f"Sizes file, {chrom_sizes_file}, not found or is `None`")
    sizes = {}
    with open(chrom_sizes_file, "r", encoding="utf-8") as handle:
        for line in handle:
            if not line.strip():
                continue
            fields = line.rstrip("\n").split("\t")
            sizes[fields[0]] = int(fields[1])
    return sizes


def check_type_bam_files(bam_files) -> list:
    """rocco/readtracks.py:636-652: a list of BAM paths, or a text file naming one per line; every path must exist."""
    if isinstance(bam_files, str):
        with open(bam_files, "r") as handle:
            bam_files_ = [line.strip() for line in handle if line.strip()]
        for file_ in bam_files_:
            if not os.path.exists(file_):
                raise FileNotFoundError(f"File in `bam_files_` not found: {file_}")
    elif isinstance(bam_files, list):
        bam_files_ = bam_files
        for file_ in bam_files_:
            if not os.path.exists(file_):
                raise FileNotFoundError(f"File in `bam_files` not found: {file_}")
    else:
        raise ValueError("`bam_files` must be either a list or a path to a text file containing a list of BAM file paths.")
    return bam_files_


def get_bam_chrom_reads(bam_file, *_args, **_kwargs):
    """The reference counts reads here through htslib (rocco/readtracks.py:389-518 over rocco/_hts_counts.c): BAM decoding
    is out of this package's scope.  ``generate_chrom_matrix`` looks this name up in the
    module when it is called, so an integrator puts the reference's reader (or any ``(starts, values)`` source) here."""
    raise RuntimeError("rocco_amd does not decode BAM files: replace rocco_amd.readtracks.get_bam_chrom_reads with the "
                       f"reference's reader (asked for {bam_file}); a reader that decodes the records itself binds "
                       "rocco_amd.readtracks.bam_chrom_reads_from_records behind it, which does the rest on the device")


def get_bigwig_chrom_scores(bigwig_file: str, chromosome: str, chrom_sizes_file: str, const_scale: float = 1.0,
                            round_digits: int = 5):
    """rocco/readtracks.py:94-186 with the same arguments, return value and errors: pyBigWig (when installed) hands back the
    chromosome's intervals; validation, dense fill of the fixed-step grid, scaling and rounding run on the device
    (`bigwig_dense_fill`).  Pinned by tests/golden/assemble_vectors.npz, which the reference's own function wrote over a
    stand-in pyBigWig object."""
    if not os.path.exists(bigwig_file):
        raise FileNotFoundError(f"bigWig file not found: {bigwig_file}")
    if not os.path.exists(chrom_sizes_file):
        raise FileNotFoundError(f"Chromosome sizes file not found: {chrom_sizes_file}")
    if chromosome not in get_chroms_and_sizes(chrom_sizes_file):
        raise ValueError(f"Chromosome {chromosome} not found in chromosome sizes file: {chrom_sizes_file}")
    bw = _require_pybigwig().open(bigwig_file)
    if bw is None:
        raise RuntimeError(f"Could not open bigWig file: {bigwig_file}...try installing `pyBigWig`: `python -m pip install pybigwig`")
    try:
        if chromosome not in bw.chroms():
            logger.warning("Chromosome %s not found in bigWig file: %s. Returning (None,None).", chromosome, bigwig_file)
            return None, None
        intervals_raw = bw.intervals(chromosome)
    finally:
        bw.close()
    if intervals_raw is None or len(intervals_raw) == 0:
        logger.warning("No intervals found in bigWig file: %s for chromosome: %s. Returning (None,None).", bigwig_file, chromosome)
        return None, None
    starts = np.asarray([int(entry[0]) for entry in intervals_raw], dtype=np.int64)
    ends = np.asarray([int(entry[1]) for entry in intervals_raw], dtype=np.int64)
    vals = np.asarray([float(entry[2]) for entry in intervals_raw], dtype=np.float64)
    if const_scale == 0:
        logger.warning("You are scaling the values by 0.")
    return bigwig_dense_fill(starts, ends, vals, const_scale=const_scale, round_digits=round_digits, bigwig_file=bigwig_file,
                             chromosome=chromosome)


def generate_chrom_matrix(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, const_scale: float = 1.0,
                          round_digits: int = 5, scale_by_step: bool = False, effective_genome_size: float = -1,
                          norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                          extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                          num_processors: int = -1, low_memory: bool = False):
    """rocco/readtracks.py:521-633 with the same signature: one ``(starts, values)`` list per input file from the per-file
    reader of its type (`get_bam_chrom_reads` / `get_bigwig_chrom_scores`, looked up in this module when called, with the
    reference's positional arguments), files without data excluded, ``(None, None)`` when none has any; then the union
    of starts, the bigWig fixed-step check and the dense K x m matrix on the device (`assemble_chrom_matrix`).  The
    readers run one after the other in this process (one process per GPU: no fork pool behind an initialised device).
    Pinned by tests/golden/assemble_vectors.npz, written by the reference's own function with its readers replaced."""
    track_types = {_get_track_type(input_file) for input_file in input_files}
    if len(track_types) != 1:
        raise ValueError("All input files must share the same type.")
    track_type = next(iter(track_types))
    threads = max((os.cpu_count() or 2) - 1, 1) if (num_processors is None or int(num_processors) < 1) else int(num_processors)
    reads = globals()
    if track_type == "bam":
        count_results = [reads["get_bam_chrom_reads"](input_file, chromosome, chrom_sizes_file, step, effective_genome_size, norm_method,
                                                      min_mapping_score, flag_include, flag_exclude, extend_reads, center_reads,
                                                      ignore_for_norm, scale_factor, threads, const_scale, round_digits, scale_by_step)
                         for input_file in input_files]
    else:
        count_results = [reads["get_bigwig_chrom_scores"](input_file, chromosome, chrom_sizes_file, const_scale, round_digits)
                         for input_file in input_files]
    interval_matrix, vals_matrix = [], []
    for input_file, (intervals_, vals_) in zip(input_files, count_results):
        if intervals_ is None or vals_ is None:
            logger.warning(f"No data found for {input_file} in chromosome {chromosome}. Excluding this track for {chromosome}.")
            continue
        interval_matrix.append(intervals_)
        vals_matrix.append(vals_)
    if len(interval_matrix) == 0:
        logger.warning(f"No data found in the files {str(input_files)} for chromosome {chromosome}. Returning (None,None).")
        return None, None
    return assemble_chrom_matrix(interval_matrix, vals_matrix, track_type=track_type, low_memory=low_memory, chromosome=chromosome)
