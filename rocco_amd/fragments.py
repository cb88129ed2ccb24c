"""Count fragments files on the device (note (34)): the reference's third counting source,
``ccounts_sourceKindFragments`` (rocco/native/ccounts_backend.c) -- ``fragments.tsv.gz`` with its ``.tbi`` beside it, lines
``contig<TAB>start<TAB>end<TAB>barcode<TAB>count``, BGZF-compressed and tabix-indexed, optionally filtered by a barcode
allow-list -- under the four count modes ``coverage``, ``cutsite``, ``fiveprime`` and ``center``.

The container is read on the host (`rocco_amd.tabix_index`, the BGZF front of `rocco_amd.bam`); the blocks of a contig's span
are inflated on the host or in HIP (``inflate="host"`` / ``"device"``); everything after the inflate runs on the device
(csrc/fragments_file.hip): the text to lines, the lines to integers and barcode verdicts, those to bins.  One fragments file
and K allow-lists (one per cluster) become a K-row pseudo-bulk count matrix without the text leaving the device
(`generate_chrom_matrix_device`); the file is inflated and split into lines once for all K.

Read: the dialect of DESIGN.md note (34) -- what tabix's own parser and the reference's strict parser read alike.  A span
that leaves it is a ValueError naming the file, the contig, the line and the rule; there is no CPU fallback.

Which barcodes a file holds, how many lines each has and how many cells an allow-list really matches (row f14, note (35);
csrc/barcode_census.hip): `barcode_census` walks the whole file once on the device and returns a `BarcodeCensus`;
`get_fragments_cell_count` is the reference's ``ccounts_getCellCount``; `BarcodeCensus.write_allowlist` writes the list that
`FragmentsSource` reads back -- cell calling by fragments per barcode without a second tool or a second inflate.

Not read: ``.csi`` and ``.tbi.csi`` indexes, plain-gzip files, the reference's unused ``barcodeTag`` /
``barcodeGroupMapFile``, tabix presets other than BED."""
from __future__ import annotations

import collections
import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import bam as _bam
from . import bam_index as _bai
from . import dp as _dp
from . import readtracks as _rt
from . import tabix_index as _tbx

logger = _rt.logger

DEFAULT_BATCH_BYTES = 1 << 30        # inflated bytes of one group of `read_fragments_spans` (a choice, not a measurement)
DEFAULT_SLAB_BYTES = 64 << 20        # inflated bytes of one slab of the whole-file mapped count
FRAGMENTS_CACHE_BYTES = 4 << 30      # the budget of the decoded spans kept on the device; least recently used leave first
ALLOWLIST_LINE_BYTES = 4096          # the reference reads an allow-list with fgets into this many bytes (237)

COUNT_MODES = {"coverage": 0, "cov": 0, "0": 0, "cutsite": 1, "cut": 1, "cutsites": 1, "1": 1, "fiveprime": 2, "five_prime": 2, "5p": 2,
               "2": 2, "center": 3, "centre": 3, "midpoint": 3, "3": 3}  # rocco/_hts_counts.c:37-80
MODE_COVERAGE, MODE_CUTSITE, MODE_FIVEPRIME, MODE_CENTER = range(4)

META, FIELDS_SHIFT, FIELDS_MASK = 0x1, 1, 0x7
START_OK, END_OK, LAST_EMPTY, FIFTH_EMPTY, WEIGHT_PARSED, BARCODE_PRESENT, BARCODE_ALLOWED, NONCANONICAL, BEYOND = (
    0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800, 0x1000)
ERR_FIELDS, ERR_NUL, ERR_CR, ERR_NONCANONICAL, ERR_BEYOND, ERR_COUNT, ERR_CONTIG, ERR_ORDER = range(1, 9)
_ERROR_TEXT = {
    ERR_FIELDS: "it has fewer than three fields",
    ERR_NUL: "it holds a NUL byte",
    ERR_CR: "it holds a carriage return that does not stand directly before its line feed",
    ERR_NONCANONICAL: "its column 2 or 3 is no canonical decimal (`0` or `[1-9][0-9]*`): tabix and the counter would read two different numbers",
    ERR_BEYOND: "its column 2 or 3 lies at or beyond 2**31",
    ERR_COUNT: "its column 5 has more than 18 digits or lies at or beyond 2**31",
    ERR_CONTIG: "its column 1 is not the contig the index names for this span",
    ERR_ORDER: "its column 2 lies below that of the line before it: the file is not sorted by begin",
}
_INDEX_RULES = (ERR_CONTIG, ERR_ORDER)  # (a line that breaks one of these: the index does not describe its file)


class _LoadCounts:
    """How often this module inflated spans, split text into lines and parsed fields (what the tests count decodes by)."""
    inflates = lines = fields = 0


def parse_count_mode(count_mode) -> int:
    """rocco/_hts_counts.c:37-80: the reference's spellings of the four modes; ValueError for anything else."""
    mode = COUNT_MODES.get(count_mode) if isinstance(count_mode, str) else None
    if mode is None:
        raise ValueError(f"unsupported count mode `{count_mode}`")
    return mode


# --------------------------------------------------------------------------------------------
# sources and allow-lists
# --------------------------------------------------------------------------------------------

def parse_barcode_allowlist(raw: bytes, name: str = "<bytes>") -> Tuple[np.ndarray, np.ndarray]:
    """The entries of an allow-list file under the reference's rules (ccounts_backend.c:237-299), sorted as ``strcmp`` sorts
    them, duplicates dropped, packed: (the entries' bytes one behind the other as uint8, the n + 1 offsets as int64).  Per
    line: leading whitespace is skipped, an empty line or one that begins with ``#`` is skipped, the entry runs to the first
    whitespace.  ValueError for a line that does not fit the reference's 4 096-byte buffer (``fgets`` reads 4 095 bytes at a
    time, the line feed among them: a longer line would be read in pieces; an unterminated last line may have 4 095 bytes) and
    for a NUL byte."""
    entries = set()
    pieces = raw.split(b"\n")
    for number, line in enumerate(pieces):
        size = len(line) + (1 if number < len(pieces) - 1 else 0)  # (with its line feed, where it has one)
        if size > ALLOWLIST_LINE_BYTES - 1:
            raise ValueError(f"{name}: line {number + 1} of the barcode allow-list has {size} bytes: the reference reads it "
                             f"through a buffer of {ALLOWLIST_LINE_BYTES} bytes, in pieces")
        if b"\x00" in line:
            raise ValueError(f"{name}: line {number + 1} of the barcode allow-list holds a NUL byte")
        token = line.lstrip(b" \t\n\v\f\r")
        if not token or token.startswith(b"#"):
            continue
        entries.add(token.split(None, 1)[0] if token.split(None, 1) else token)
    ordered = sorted(entries)
    offsets = np.zeros(len(ordered) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in ordered], out=offsets[1:])
    return np.frombuffer(b"".join(ordered), dtype=np.uint8).copy(), offsets


def load_barcode_allowlist(path) -> Tuple[np.ndarray, np.ndarray]:
    """`parse_barcode_allowlist` of a file; RuntimeError with the reference's words where it does not open."""
    try:
        with open(os.fspath(path), "rb") as handle:
            raw = handle.read()
    except OSError:
        raise RuntimeError("failed to open barcode allowlist") from None
    return parse_barcode_allowlist(raw, os.fspath(path))


_NO_LIST = (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))


class FragmentsSource:
    """A fragments file and, optionally, the barcodes that count: ``path`` (``.tsv.gz``, BGZF, with ``<path>.tbi``),
    ``barcode_allowlist_file`` (one barcode per line; None or "" for none).  Every function of this module that takes a
    path takes one of these too."""

    def __init__(self, path, barcode_allowlist_file=None):
        self.path = os.fspath(path)
        self.barcode_allowlist_file = os.fspath(barcode_allowlist_file) if barcode_allowlist_file else None
        self._allow = (None, None)  # (the list as loaded, under the file's (path, size, mtime) at that time)

    def allow_key(self):
        if not self.barcode_allowlist_file:
            return None
        try:
            return _bam._file_key(self.barcode_allowlist_file)
        except OSError:
            raise RuntimeError("failed to open barcode allowlist") from None

    def allowlist(self) -> Tuple[np.ndarray, np.ndarray]:
        """The packed list; read again where the file has changed since (the cached lines key on the same (size, mtime))."""
        if not self.barcode_allowlist_file:
            return _NO_LIST
        key = self.allow_key()
        if self._allow[0] != key:
            self._allow = (key, load_barcode_allowlist(self.barcode_allowlist_file))
        return self._allow[1]

    def __fspath__(self) -> str:
        return self.path

    def __repr__(self) -> str:
        return f"FragmentsSource({self.path!r}, barcode_allowlist_file={self.barcode_allowlist_file!r})"


def _as_source(source) -> FragmentsSource:
    return source if isinstance(source, FragmentsSource) else FragmentsSource(source)


def _index_of(source: FragmentsSource) -> _tbx.TabixIndex:
    index = _tbx.open_tabix_index(source.path)
    if index is None:
        raise RuntimeError(f"failed to load tabix index for fragments source: {source.path}")
    return index


# --------------------------------------------------------------------------------------------
# the kernels through the C ABI
# --------------------------------------------------------------------------------------------

def fragfile_shape() -> dict:
    """`rocco_hip_fragfile_shape`: the sizes at which the kernels take a second turn.  No device is touched."""
    shape = (ctypes.c_int * 6)()
    _native.load().rocco_hip_fragfile_shape(shape)
    return {"threads": int(shape[0]), "tile_bytes": int(shape[1]), "lines_per_turn": int(shape[2]), "lines_max_grid": int(shape[3]),
            "fields_max_grid": int(shape[4]), "count_max_grid": int(shape[5])}


def _ll(values) -> np.ndarray:
    return np.ascontiguousarray(values, dtype=np.int64)


def _ll_p(array: np.ndarray):
    return array.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))


def _names_table(names: Sequence[str]):
    packed = [n.encode("utf-8", "surrogateescape") if isinstance(n, str) else bytes(n) for n in names]
    offsets = np.zeros(len(packed) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in packed], out=offsets[1:])
    return np.frombuffer(b"".join(packed) + b"\x00", dtype=np.uint8).copy(), offsets


def _pack_allowlists(allowlists):
    """K packed lists as one: (the K + 1 first entries, the n + 1 offsets into the bytes, the bytes -- never empty, at their
    exact size otherwise --, n)."""
    allow_first, allow_offsets, allow_bytes, entries, at = [0], [], [], 0, 0
    for packed, offsets in allowlists:
        allow_offsets.append(np.asarray(offsets[:-1], dtype=np.int64) + at)
        allow_bytes.append(np.asarray(packed, dtype=np.uint8))
        entries += len(offsets) - 1
        at += int(offsets[-1])
        allow_first.append(entries)
    allow_offsets = np.concatenate(allow_offsets + [np.asarray([at], dtype=np.int64)])
    return allow_first, allow_offsets, np.concatenate(allow_bytes + [np.zeros(1, dtype=np.uint8)])[: max(at, 1)], entries


def lines_device(bytes_t, entry0: int = 0, n_bytes: Optional[int] = None):
    """`rocco_hip_fragfile_lines` over a uint8 CUDA tensor: (the n_lines + 1 line starts as an int64 CUDA tensor, the report
    ``lines``, ``cut`` (the offset behind the last line feed) and ``open`` (the last line is unterminated))."""
    import torch

    lib = _native.load()
    if not _dp._is_tensor(bytes_t) or bytes_t.dtype != torch.uint8 or bytes_t.dim() != 1 or not bytes_t.is_cuda:
        raise TypeError("lines_device: a one-dimensional uint8 CUDA tensor is required")
    bytes_t = bytes_t.contiguous()
    n = int(bytes_t.shape[0]) if n_bytes is None else int(n_bytes)
    solver, stream = _native.solver_for(bytes_t.device.index).handle, _dp._stream_ptr(bytes_t)
    back = (ctypes.c_longlong * 4)()
    _native.check(lib.rocco_hip_fragfile_lines(solver, bytes_t.data_ptr(), n, int(entry0), None, 0, back, stream), "rocco_hip_fragfile_lines")
    starts = torch.empty(int(back[0]) + 1, dtype=torch.int64, device=bytes_t.device)
    _native.check(lib.rocco_hip_fragfile_lines(solver, bytes_t.data_ptr(), n, int(entry0), starts.data_ptr(), int(starts.shape[0]), back, stream),
                  "rocco_hip_fragfile_lines")
    _LoadCounts.lines += 1
    return starts, {"lines": int(back[0]), "cut": int(back[1]), "open": bool(back[2])}


class FragmentLines:
    """The parsed lines of one span (or slab): ``start``, ``end``, ``weight``, ``name`` (int32 CUDA tensors) and ``status``
    (the status words, as int32 bit patterns), in file order."""

    __slots__ = ("start", "end", "weight", "name", "status")

    def __init__(self, start, end, weight, name, status):
        self.start, self.end, self.weight, self.name, self.status = start, end, weight, name, status

    def __len__(self) -> int:
        return int(self.start.shape[0])

    def nbytes(self) -> int:
        return 20 * len(self)

    def slice(self, lo: int, hi: int) -> "FragmentLines":
        return FragmentLines(*[getattr(self, f)[lo:hi] for f in self.__slots__])


def _empty_lines(dev) -> FragmentLines:
    import torch

    return FragmentLines(*[torch.empty(0, dtype=torch.int32, device=dev) for _ in FragmentLines.__slots__])


def fields_device(bytes_t, starts_t, whole_file: bool, track_first: Sequence[int], expect: Sequence[int], names: Sequence[str],
                  allowlists: Sequence[Tuple[np.ndarray, np.ndarray]], n_bytes: Optional[int] = None):
    """`rocco_hip_fragfile_fields`: (`FragmentLines` of all lines, (first offending line or -1, its lowest code)).
    ``track_first``: the K + 1 line offsets of the tracks; ``expect[k]``: the index among ``names`` that column 1 of track k's
    lines must have (-1: any); ``allowlists[k]``: the packed, sorted allow-list of track k (`parse_barcode_allowlist`)."""
    import torch

    lib = _native.load()
    dev = bytes_t.device
    bytes_t, starts_t = bytes_t.contiguous(), starts_t.contiguous()
    n_lines, K = int(starts_t.shape[0]) - 1, len(expect)
    if n_lines < 0 or len(track_first) != K + 1 or len(allowlists) != K:
        raise ValueError("fields_device: n_lines + 1 starts, K + 1 track offsets and K allow-lists are required")
    out = FragmentLines(*[torch.empty(n_lines, dtype=torch.int32, device=dev) for _ in FragmentLines.__slots__])
    name_bytes, name_offsets = _names_table(names)
    allow_first, allow_offsets, allow_bytes, entries = _pack_allowlists(allowlists)
    with torch.cuda.device(dev):
        allow_bytes_t = torch.from_numpy(allow_bytes).to(dev)
        allow_offsets_t = torch.from_numpy(allow_offsets).to(dev)
        first_a, allow_first_a, expect_a = _ll(track_first), _ll(allow_first), np.ascontiguousarray(expect, dtype=np.int32)
        back = (ctypes.c_longlong * 4)()
        _native.check(lib.rocco_hip_fragfile_fields(
            _native.solver_for(dev.index).handle, bytes_t.data_ptr(), int(bytes_t.shape[0]) if n_bytes is None else int(n_bytes),
            starts_t.data_ptr(), n_lines, 1 if whole_file else 0, _ll_p(first_a), expect_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), K,
            name_bytes.ctypes.data, _ll_p(name_offsets), len(names), allow_bytes_t.data_ptr(), allow_offsets_t.data_ptr(), entries,
            _ll_p(allow_first_a), out.start.data_ptr(), out.end.data_ptr(), out.weight.data_ptr(), out.name.data_ptr(), out.status.data_ptr(),
            back, _dp._stream_ptr(bytes_t)), "rocco_hip_fragfile_fields")
    _LoadCounts.fields += 1
    return out, (int(back[0]), int(back[1]))


class _ModeOptions(ctypes.Structure):
    _fields_ = [("count_mode", ctypes.c_int32), ("one_read_per_bin", ctypes.c_int32)]


def _cat_lines(lines_list: Sequence[FragmentLines], fields: Sequence[str], dev):
    """The tracks' line arrays back to back and the K + 1 offsets (a single track is used where it lies)."""
    import torch

    offsets = [0]
    for lines in lines_list:
        offsets.append(offsets[-1] + len(lines))
    if len(lines_list) == 1:
        return {f: getattr(lines_list[0], f).contiguous() for f in fields}, offsets
    return {f: torch.cat([getattr(lines, f) for lines in lines_list]) if offsets[-1] else torch.empty(0, dtype=torch.int32, device=dev)
            for f in fields}, offsets


def count_lines_batch_device(lines_list: Sequence[FragmentLines], regions: Sequence, modes: Sequence, one_read_per_bin: Sequence,
                             lengths: Optional[Sequence[Optional[int]]] = None, check: bool = True):
    """`rocco_hip_fragfile_count_batch`: ``ccounts_countRegion``'s fragments branch (ccounts_backend.c:2212-2353) for K tracks
    in one launch series.  ``regions[k]``: (start, end, step); ``modes[k]``: a count mode as `parse_count_mode` reads it or its
    number; ``lengths[k]``: the reference's countBufferLength where it is not ((end - start - 1) // step) + 1.  Returns (one
    float32 CUDA tensor per track, the largest magnitude per track); RuntimeError beyond 2**24 unless ``check`` is False."""
    import torch

    lib = _native.load()
    K = len(lines_list)
    if K == 0 or len(regions) != K or len(modes) != K or len(one_read_per_bin) != K:
        raise ValueError("one region, one mode and one one_read_per_bin per track are required")
    dev = lines_list[0].start.device
    regs, opts, out_offsets, total = (_rt.CountRegion * K)(), (_ModeOptions * K)(), np.zeros(K, dtype=np.int64), 0
    for k, region in enumerate(regions):
        start, end, step = (int(v) for v in region)
        if step <= 0 or end <= start:
            raise ValueError("invalid interval size or genomic segment")  # (the reference's wording, rocco/_hts_counts.c:500-506)
        if start < 0 or end >= _rt.POSITION_LIMIT:
            raise ValueError("a region must lie in [0, 2**31)")
        bins = ((end - start - 1) // step) + 1 if lengths is None or lengths[k] is None else int(lengths[k])
        if bins <= 0:
            raise ValueError("a track needs at least one bin")
        regs[k] = _rt.CountRegion(start, end, step, bins)
        opts[k] = _ModeOptions(modes[k] if isinstance(modes[k], int) else parse_count_mode(modes[k]), 1 if one_read_per_bin[k] else 0)
        out_offsets[k] = total
        total += (bins + 3) // 4 * 4
    with torch.cuda.device(dev):
        cat, offsets = _cat_lines(lines_list, ("start", "end", "weight", "status"), dev)
        out = torch.empty(total, dtype=torch.float32, device=dev)
        maxima, line_offsets = (ctypes.c_longlong * K)(), _ll(offsets)
        _native.check(lib.rocco_hip_fragfile_count_batch(
            _native.solver_for(dev.index).handle, cat["start"].data_ptr(), cat["end"].data_ptr(), cat["weight"].data_ptr(),
            cat["status"].data_ptr(), _ll_p(line_offsets), K, ctypes.cast(opts, ctypes.c_void_p), ctypes.cast(regs, ctypes.c_void_p),
            _ll_p(out_offsets), out.data_ptr(), maxima, _dp._stream_ptr(out)), "rocco_hip_fragfile_count_batch")
    maxima = [int(m) for m in maxima]
    if check:
        _rt._check_exact_counts(maxima)
    return [out[int(out_offsets[k]): int(out_offsets[k]) + regs[k].n_bins] for k in range(K)], maxima


def chrom_ranges_batch_device(lines_list: Sequence[FragmentLines], chrom_sizes: Sequence[int]) -> List[Tuple[int, int]]:
    """`rocco_hip_fragfile_chrom_range_batch`: ``ccounts_getChromRange``'s fragments branch (1583-1631) per track: (start of
    the first valid line, end of the LAST valid line in file order) among the lines that begin below ``chrom_sizes[k]``,
    (0, 0) where there is none."""
    import torch

    K = len(lines_list)
    dev = lines_list[0].start.device
    with torch.cuda.device(dev):
        cat, offsets = _cat_lines(lines_list, ("start", "end", "status"), dev)
        ranges, line_offsets, limits = (ctypes.c_longlong * (2 * K))(), _ll(offsets), _ll([int(c) for c in chrom_sizes])
        _native.check(_native.load().rocco_hip_fragfile_chrom_range_batch(
            _native.solver_for(dev.index).handle, cat["start"].data_ptr(), cat["end"].data_ptr(), cat["status"].data_ptr(),
            _ll_p(line_offsets), _ll_p(limits), K, ranges, _dp._stream_ptr(cat["start"])), "rocco_hip_fragfile_chrom_range_batch")
    return [(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(K)]


def mapped_count_device(lines: FragmentLines, mode: int, one_read_per_bin: int) -> int:
    """`rocco_hip_fragfile_mapped_count` over the lines of a whole-file field pass."""
    import torch

    total = ctypes.c_uint64(0)
    dev = lines.start.device
    with torch.cuda.device(dev):
        _native.check(_native.load().rocco_hip_fragfile_mapped_count(
            _native.solver_for(dev.index).handle, lines.weight.data_ptr(), lines.name.data_ptr(), lines.status.data_ptr(), len(lines),
            int(mode), 1 if one_read_per_bin else 0, ctypes.byref(total), _dp._stream_ptr(lines.weight)), "rocco_hip_fragfile_mapped_count")
    return int(total.value)


def fragfile_host(data, entry0: int = 0, whole_file: bool = False, track_first: Optional[Sequence[int]] = None, expect: Sequence[int] = (-1,),
                  names: Sequence[str] = (), allowlists: Sequence[Tuple[np.ndarray, np.ndarray]] = (_NO_LIST,), fields: bool = True) -> dict:
    """`rocco_hip_fragfile_host`: the line pass and the field pass over host bytes on the calling thread, every array at its
    exact size (test support).  Returns ``starts``, ``lines``, ``cut``, ``open`` and, with ``fields``, ``start``, ``end``,
    ``weight``, ``name``, ``status`` (uint32) and ``report`` (first offending line or -1, its lowest code)."""
    lib = _native.load()
    raw = np.frombuffer(bytes(data), dtype=np.uint8).copy() if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    back = (ctypes.c_longlong * 4)()
    none = [None] * 5
    ptr = raw.ctypes.data if raw.size else None
    _native.check(lib.rocco_hip_fragfile_host(None, ptr, raw.size, int(entry0), None, 0, back, 0, None, None, 0, None, None, 0, None, None, 0,
                                              None, *none, None), "rocco_hip_fragfile_host")
    n_lines = int(back[0])
    starts = np.empty(n_lines + 1, dtype=np.int64)
    out = {"lines": n_lines, "cut": int(back[1]), "open": bool(back[2]), "starts": starts}
    K = len(expect)
    name_bytes, name_offsets = _names_table(names)
    allow_first, allow_offsets, allow_bytes, entries = _pack_allowlists(allowlists)
    arrays = [np.empty(n_lines, dtype=np.int32) for _ in range(4)] + [np.empty(n_lines, dtype=np.uint32)]
    report = (ctypes.c_longlong * 4)()
    first_a = None if track_first is None else _ll(track_first)
    allow_first_a, expect_a = _ll(allow_first), np.ascontiguousarray(expect, dtype=np.int32)
    outs = [a.ctypes.data for a in arrays] if fields else none
    _native.check(lib.rocco_hip_fragfile_host(
        None, ptr, raw.size, int(entry0), starts.ctypes.data, starts.size, back, 1 if whole_file else 0,
        None if first_a is None else _ll_p(first_a), expect_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), K, name_bytes.ctypes.data,
        _ll_p(name_offsets), len(names), allow_bytes.ctypes.data, allow_offsets.ctypes.data, entries, _ll_p(allow_first_a), *outs,
        report if fields else None), "rocco_hip_fragfile_host")
    if fields:
        out.update(dict(zip(("start", "end", "weight", "name", "status"), arrays)), report=(int(report[0]), int(report[1])))
    return out


# --------------------------------------------------------------------------------------------
# spans of (source, contig) pairs through the index
# --------------------------------------------------------------------------------------------

class _Stream:
    """One (file, contig) of `read_fragments_spans`, with what `rocco_amd.bam._group_bytes_device` / `_host` read of it."""

    __slots__ = ("path", "contig", "tid", "raw", "blocks", "skip", "keep", "size", "index_name", "key")

    def where(self) -> str:
        return f"{self.path}: contig {self.contig}"


def _line_error(stream: "_Stream", ordinal: int, code: int) -> ValueError:
    text = f"{stream.where()}: line {ordinal} of its span: {_ERROR_TEXT.get(code, f'error {code}')}"
    if code in _INDEX_RULES:
        text += f"; the index {stream.index_name} does not describe this file"
    return ValueError(text)


_TEXT_CACHE: "collections.OrderedDict" = collections.OrderedDict()    # (file key, contig) -> (group bytes, the span's starts, bytes kept)
_LINES_CACHE: "collections.OrderedDict" = collections.OrderedDict()   # (file key, contig, allow-list key) -> FragmentLines


def clear_fragments_cache() -> None:
    """Drops every decoded span (and the metadata derived from whole files)."""
    _TEXT_CACHE.clear()
    _LINES_CACHE.clear()
    _FRAGMENTS_COUNT_METADATA_CACHE.clear()


def _evict() -> None:
    def held() -> int:
        return sum(v[2] for v in _TEXT_CACHE.values()) + sum(v.nbytes() for v in _LINES_CACHE.values())

    while held() > FRAGMENTS_CACHE_BYTES and (_LINES_CACHE or _TEXT_CACHE):
        (_LINES_CACHE if _LINES_CACHE else _TEXT_CACHE).popitem(last=False)


def _stream_of(source: FragmentsSource, contig: str, raws: dict) -> Optional["_Stream"]:
    """The stream of a pair, None for a contig the index does not know."""
    index = _index_of(source)
    if contig not in index.tid_of:
        return None
    s = _Stream()
    s.path, s.contig, s.tid, s.index_name = source.path, contig, index.tid_of[contig], index.name
    s.key = (_bam._file_key(source.path), contig)
    s.raw, s.blocks, s.skip, s.keep, s.size = None, [], 0, 0, 0
    span = _bai.contig_span(index, s.tid)
    if span is not None:
        if source.path not in raws:
            raws[source.path] = _bam._mapped_bytes(source.path)
        s.raw = raws[source.path]
        s.blocks, s.skip, s.keep = _bam._bgzf_span_blocks(s.raw, source.path, contig, span[0], span[1])
        if s.blocks:
            s.size = sum(b[4] for b in s.blocks) - s.skip - (s.blocks[-1][4] - s.keep)
            if s.size < 0:
                raise ValueError(f"{s.where()}: its span ends at virtual offset {span[1]}, before its begin {span[0]}; the index "
                                 f"{s.index_name} does not describe this file")
    return s


def span_bytes_host(source, contig: str) -> Optional[bytes]:
    """The inflated text of a contig's span, on the host (test support; no device is touched): None for a contig the index
    does not know, ``b""`` for one without a span."""
    s = _stream_of(_as_source(source), str(contig), {})
    if s is None:
        return None
    parts = []
    for index, block in enumerate(s.blocks):
        data = _bam._inflate_block(s.raw, s.path, index, block)
        parts.append(data[s.skip if index == 0 else 0: s.keep if index == len(s.blocks) - 1 else len(data)])
    return b"".join(parts)


def _ends_file(s: "_Stream") -> bool:
    """Whether the stream takes the whole of its last block and at most an end-of-file marker (28 bytes) follows that."""
    return bool(s.blocks) and s.keep == s.blocks[-1][4] and s.blocks[-1][2] + 8 + 28 >= len(s.raw)


def _decode_group(group: List["_Stream"], sources: List[FragmentsSource], dev, inflate: str, threads: Optional[int]) -> None:
    """One inflate, one line pass and one field pass (each stream under its source's allow-list) for the streams of a group,
    laid one behind the other.  Every stream's text goes into the cache as (its own bytes, its own n + 1 line starts): of a
    group of several streams each gets a copy of its part, so that a cache entry owns what it is charged for and frees it
    when it leaves."""
    import torch

    data = _bam._group_bytes_device(group, dev) if inflate == "device" else _bam._group_bytes_host(group, dev, threads)
    _LoadCounts.inflates += 1
    bounds = np.zeros(len(group) + 1, dtype=np.int64)
    np.cumsum([s.size for s in group], out=bounds[1:])
    if int(data.shape[0]) != int(bounds[-1]):
        raise RuntimeError(f"read_fragments_spans: {int(data.shape[0])} bytes laid out where the spans hold {int(bounds[-1])}")
    starts, report = lines_device(data)
    # where every stream's lines begin: its first byte must be a line start (the stream before it ends behind a line feed)
    bounds_t = torch.from_numpy(bounds).to(dev)
    first = torch.searchsorted(starts, bounds_t).cpu().numpy()
    found = starts[torch.from_numpy(np.minimum(first, report["lines"])).to(dev)].cpu().numpy()
    for k, s in enumerate(group):
        if s.size and int(found[k]) != int(bounds[k]):
            raise ValueError(f"{group[k - 1].where()}: its span ends inside a line; the index {group[k - 1].index_name} does not describe this file")
    views = [starts[int(first[k]): int(first[k + 1]) + 1] for k in range(len(group))]
    _fields_pass(data, views, group, sources)
    for k, s in enumerate(group):
        own = (data, views[k]) if len(group) == 1 else (data[int(bounds[k]): int(bounds[k + 1])].clone(), views[k] - int(bounds[k]))
        _TEXT_CACHE[s.key] = own + (int(s.size) + 8 * int(views[k].shape[0]),)


def read_fragments_spans(wanted, device=None, inflate: Optional[str] = None, batch_bytes: int = DEFAULT_BATCH_BYTES,
                         threads: Optional[int] = None) -> List[Optional[FragmentLines]]:
    """The parsed lines of every ``(source, contig)`` of ``wanted`` -- several contigs of one file, one contig of K sources,
    K allow-lists over one file, any mix -- through the files' ``.tbi`` indexes: one `FragmentLines` per pair (``status``
    carries the verdict of the pair's own allow-list), None for a contig its index does not know, empty lines for a contig
    without a span.  Only the BGZF blocks between the virtual offsets the index names are read.

    The streams that are not yet on the device are grouped under ``batch_bytes`` inflated bytes; a group costs one inflate
    (``inflate="device"``: one block table, one upload, one `rocco_hip_bgzf_inflate`; ``"host"``: the thread pool places every
    block's useful bytes in one pinned buffer, one upload; default `rocco_amd.bam.DEFAULT_INFLATE`), one line pass and one
    field pass, each stream under the allow-list of the first pair that asks for it; a further allow-list over the same
    stream costs a field pass of its own, no inflate.  Text and lines stay on the device under `FRAGMENTS_CACHE_BYTES`.
    RuntimeError with the reference's words for a file without a ``.tbi``; ValueError naming file, contig, line and rule
    for a line outside the dialect."""
    import torch

    inflate = _bam.DEFAULT_INFLATE if inflate is None else inflate
    if inflate not in ("host", "device"):
        raise ValueError(f"read_fragments_spans: inflate must be \"host\" or \"device\", not {inflate!r}")
    if int(batch_bytes) < 1:
        raise ValueError("read_fragments_spans: batch_bytes must be positive")
    dev = _dp._device(device)
    pairs = [(_as_source(source), str(contig)) for source, contig in wanted]
    raws, streams = {}, []
    for source, contig in pairs:
        streams.append(_stream_of(source, contig, raws))
    with torch.cuda.device(dev):
        # 1. the text of every stream that is not on the device
        todo, seen = [], set()
        for s in streams:
            if s is not None and s.size and s.key not in seen and not (s.key in _TEXT_CACHE and _TEXT_CACHE[s.key][0].device == dev):
                seen.add(s.key)
                todo.append(s)
        groups, at = [], 0
        while at < len(todo):
            last, size = at + 1, todo[at].size
            # (a stream that reaches its file's last block may end in an unterminated line: nothing is laid behind it)
            while last < len(todo) and size + todo[last].size <= int(batch_bytes) and not _ends_file(todo[last - 1]):
                size, last = size + todo[last].size, last + 1
            groups.append(todo[at:last])
            at = last
        first_asker = {}
        for (source, contig), s in zip(pairs, streams):
            if s is not None and s.size:
                first_asker.setdefault(s.key, source)
        for group in groups:
            _decode_group(group, [first_asker[s.key] for s in group], dev, inflate, threads)
        # 2. the fields of every pair whose allow-list has not been over its stream yet: one pass each, no inflate
        out: List[Optional[FragmentLines]] = [None] * len(pairs)
        for i, ((source, contig), s) in enumerate(zip(pairs, streams)):
            if s is None:
                continue
            if not s.size:
                out[i] = _empty_lines(dev)
                continue
            key = s.key + (source.allow_key(),)
            hit = _LINES_CACHE.get(key)
            if hit is not None and hit.start.device == dev:
                _LINES_CACHE.move_to_end(key)
                out[i] = hit
                continue
            text = _TEXT_CACHE[s.key]
            _fields_pass(text[0], [text[1]], [s], [source])
            out[i] = _LINES_CACHE[key]
        _evict()
    return out


def _fields_pass(data, views, group: List["_Stream"], sources: List[FragmentsSource]) -> None:
    """One field pass over streams whose text lies one behind the other in ``data`` (``views[k]``: the n + 1 line starts of
    stream k, neighbours sharing their border entry), each under its source's allow-list; the lines go into the cache (of
    several streams each a copy of its part: an entry owns what it is charged for)."""
    import torch

    if len(group) == 1:
        starts = views[0]
    else:  # (the views are neighbouring slices of one tensor that share their border entries)
        starts = torch.cat([v[:-1] for v in views] + [views[-1][-1:]])
    track_first = np.zeros(len(group) + 1, dtype=np.int64)
    np.cumsum([int(v.shape[0]) - 1 for v in views], out=track_first[1:])
    names = sorted({s.contig for s in group})
    lines, (line, code) = fields_device(data, starts, False, track_first, [names.index(s.contig) for s in group], names,
                                        [source.allowlist() for source in sources])
    if line >= 0:
        k = int(np.searchsorted(track_first, line, side="right")) - 1
        raise _line_error(group[k], line - int(track_first[k]) + 1, code)
    for k, (s, source) in enumerate(zip(group, sources)):
        part = lines.slice(int(track_first[k]), int(track_first[k + 1]))
        _LINES_CACHE[s.key + (source.allow_key(),)] = part if len(group) == 1 else FragmentLines(*[getattr(part, f).clone() for f in part.__slots__])


# --------------------------------------------------------------------------------------------
# the reference's four entry points over a fragments source
# --------------------------------------------------------------------------------------------

def count_fragments_regions(requests: Sequence[tuple], device=None, inflate: Optional[str] = None) -> list:
    """K region counts in one launch series: ``requests[k]`` = (source, chromosome, start, end, step, count_mode,
    one_read_per_bin).  Returns one float32 CUDA tensor per request.  RuntimeError "failed to open fragments region iterator"
    for a contig the source's index does not know (ccounts_backend.c:2198-2203)."""
    lines = read_fragments_spans([(r[0], r[1]) for r in requests], device=device, inflate=inflate)
    for found, r in zip(lines, requests):
        if found is None:
            raise RuntimeError("failed to open fragments region iterator")
    counts, _ = count_lines_batch_device(lines, [(r[2], r[3], r[4]) for r in requests], [parse_count_mode(r[5]) for r in requests],
                                         [r[6] for r in requests])
    return counts


def count_fragments_region(source, chromosome: str, start: int, end: int, step: int, count_mode: str = "coverage", one_read_per_bin: int = 0,
                           device=None, inflate: Optional[str] = None) -> np.ndarray:
    """The reference's ``count_alignment_region`` over a fragments source (ccounts_backend.c:2156-2362): the float32 counts
    of ``[start, end)`` in bins of ``step`` under ``count_mode`` (the reference's spellings: `parse_count_mode`)."""
    parse_count_mode(count_mode)
    (counts,) = count_fragments_regions([(source, chromosome, start, end, step, count_mode, one_read_per_bin)], device, inflate)
    return counts.cpu().numpy()


def get_fragments_chrom_ranges(triples, device=None, inflate: Optional[str] = None) -> List[Tuple[int, int]]:
    """`get_fragments_chrom_range` of K (source, chromosome, chrom_size) triples with one range launch."""
    lines = read_fragments_spans([(t[0], t[1]) for t in triples], device=device, inflate=inflate)
    live = [k for k, found in enumerate(lines) if found is not None]
    out = [(0, 0)] * len(lines)
    if live:
        for k, found in zip(live, chrom_ranges_batch_device([lines[k] for k in live], [triples[k][2] for k in live])):
            out[k] = found
    return out


def get_fragments_chrom_range(source, chromosome: str, chrom_size: int, device=None, inflate: Optional[str] = None) -> Tuple[int, int]:
    """``ccounts_getChromRange`` over a fragments source (1563-1640): (start of the first valid line of the contig, end of its
    LAST valid line in file order) among the lines that begin below ``chrom_size`` (the reference queries [0, chrom_size));
    (0, 0) where there is none or the index does not know the contig."""
    return get_fragments_chrom_ranges([(source, chromosome, chrom_size)], device, inflate)[0]


def _whole_file_slabs(source: FragmentsSource, dev, inflate: str, slab_bytes: int, threads: Optional[int]):
    raw = _bam._mapped_bytes(source.path)
    blocks = _bam._bgzf_blocks(raw, source.path)
    if inflate == "device":
        return _bam._inflate_slabs_device(raw, source.path, blocks, dev, slab_bytes)
    return _bam._uploaded(_bam._inflate_slabs(raw, source.path, blocks, threads, slab_bytes), dev)


def get_fragments_mapped_read_count(source, exclude_chromosomes=(), count_mode: str = "coverage", one_read_per_bin: int = 0, device=None,
                                    inflate: Optional[str] = None, slab_bytes: int = DEFAULT_SLAB_BYTES,
                                    threads: Optional[int] = None) -> Tuple[int, int]:
    """``ccounts_getMappedReadCount`` over a fragments source (1751-1846): (the sum of the weights of every line of the WHOLE
    file that has a fifth field, whose contig is not excluded and whose barcode passes -- twice the weight for ``cutsite`` /
    ``fiveprime`` without ``one_read_per_bin`` --, 0).  The file goes through in slabs cut at BGZF block boundaries; the
    unfinished last line of a slab is carried into the next."""
    import torch

    source, mode = _as_source(source), parse_count_mode(count_mode)
    inflate = _bam.DEFAULT_INFLATE if inflate is None else inflate
    _index_of(source)  # (the reference opens the source with its index for this call too)
    dev = _dp._device(device)
    names = [str(c) for c in (exclude_chromosomes or ())]
    total, carry, ordinal = 0, None, 0
    with torch.cuda.device(dev):
        slabs = iter(_whole_file_slabs(source, dev, inflate, max(1, int(slab_bytes)), threads))
        slab = next(slabs, None)
        while slab is not None:
            following = next(slabs, None)
            data = slab if carry is None or not int(carry.shape[0]) else torch.cat([carry, slab])
            n, carry = int(data.shape[0]), None
            starts, report = lines_device(data)  # (one size pass and one emit pass per slab)
            n_lines = report["lines"]
            if following is not None and report["open"]:
                # cut behind the last line feed: the unfinished line (the last start is where it begins) goes in front of the next slab
                n_lines, n = n_lines - 1, report["cut"]
                starts, carry = starts[: n_lines + 1], data[n:].clone()
            if n_lines:
                lines, (line, code) = fields_device(data, starts, True, [0, n_lines], [-1], names, [source.allowlist()], n_bytes=n)
                if line >= 0:
                    raise ValueError(f"{source.path}: line {ordinal + line + 1} of the file: {_ERROR_TEXT.get(code, f'error {code}')}")
                total += mapped_count_device(lines, mode, one_read_per_bin)
                ordinal += n_lines
            slab = following
    return total, 0


# --------------------------------------------------------------------------------------------
# the barcode census: the distinct barcodes of a file and the lines of each (row f14, note (35))
# --------------------------------------------------------------------------------------------

ALL_HASH_BITS = (1 << 64) - 1
_ALLOWLIST_SPACE = b" \t\n\v\f\r"


def barcode_census_shape() -> dict:
    """`rocco_hip_barcode_census_shape`: the sizes at which the census kernels take a second turn and the smallest table.
    No device is touched."""
    shape = (ctypes.c_int * 4)()
    _native.load().rocco_hip_barcode_census_shape(shape)
    return {"threads": int(shape[0]), "lines_per_turn": int(shape[1]), "max_grid": int(shape[2]), "min_capacity": int(shape[3])}


class BarcodeCensus:
    """The distinct barcodes of a fragments file (or of some text) and how many lines each has.  ``packed``: (the barcodes'
    bytes one behind the other as uint8, the D + 1 offsets as int64), the layout of `parse_barcode_allowlist`, ordered as
    ``strcmp`` orders, bytes compared unsigned; ``barcodes``: the same as a list of ``bytes``; ``records``: int64, the lines
    per barcode; ``lines``: the lines read, with or without a barcode; ``stats``: ``capacity`` (slots of the table at the
    end), ``grows``, ``slabs``, ``entries``, ``status`` (of the last native call).  ``len()`` is the reference's cell count.
    The order is made on the host over the D distinct entries, never over the lines."""

    __slots__ = ("packed", "records", "lines", "stats", "_barcodes")

    def __init__(self, raw: np.ndarray, offsets: np.ndarray, records: np.ndarray, lines: int, stats: dict):
        raw, offsets = np.ascontiguousarray(raw, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.int64)
        found = [raw[int(offsets[e]): int(offsets[e + 1])].tobytes() for e in range(len(offsets) - 1)]
        order = sorted(range(len(found)), key=found.__getitem__)  # (bytes compare unsigned, the shorter of two first: strcmp without NUL)
        self._barcodes = [found[e] for e in order]
        sorted_offsets = np.zeros(len(order) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in self._barcodes], out=sorted_offsets[1:])
        self.packed = (np.frombuffer(b"".join(self._barcodes), dtype=np.uint8).copy(), sorted_offsets)
        self.records = np.ascontiguousarray(records, dtype=np.int64)[order] if order else np.zeros(0, dtype=np.int64)
        self.lines, self.stats = int(lines), dict(stats, entries=len(order))

    @property
    def barcodes(self) -> List[bytes]:
        return list(self._barcodes)

    def __len__(self) -> int:
        return len(self._barcodes)

    def write_allowlist(self, path, min_records: int = 1) -> int:
        """One barcode per line, those with at least ``min_records`` lines, in census order, so that
        ``FragmentsSource(file, path)`` admits exactly those.  ValueError naming the barcode for one the allow-list loader
        (`parse_barcode_allowlist`) could not read back: whitespace inside it, a leading ``#``, 4 095 bytes or more (with its
        line feed it would not fit the reference's 4 096-byte buffer).  Nothing is written then.  Returns how many it wrote."""
        kept = [b for b, n in zip(self._barcodes, self.records.tolist()) if n >= int(min_records)]
        for barcode in kept:
            why = ("it holds whitespace" if any(c in _ALLOWLIST_SPACE for c in barcode) else "it begins with `#`" if barcode.startswith(b"#") else
                   f"it has {len(barcode)} bytes, the reference's buffer of {ALLOWLIST_LINE_BYTES} takes {ALLOWLIST_LINE_BYTES - 2} and a line feed"
                   if len(barcode) >= ALLOWLIST_LINE_BYTES - 1 else "it holds a NUL byte" if b"\x00" in barcode else None)
            if why:
                shown = barcode if len(barcode) <= 64 else barcode[:64] + b"..."
                raise ValueError(f"write_allowlist: the barcode {shown!r} cannot stand in an allow-list: {why}")
        with open(os.fspath(path), "wb") as handle:
            handle.write(b"".join(b + b"\n" for b in kept))
        return len(kept)


def _census_arguments(hash_mask, initial_capacity) -> Tuple[int, int]:
    mask = ALL_HASH_BITS if hash_mask is None else int(hash_mask)
    if not 0 <= mask <= ALL_HASH_BITS:
        raise ValueError("hash_mask must be a 64-bit pattern")
    capacity = barcode_census_shape()["min_capacity"]
    if initial_capacity is not None and int(initial_capacity) < 1:
        raise ValueError("initial_capacity must be positive")
    while initial_capacity is not None and capacity < int(initial_capacity):
        capacity *= 2
    return mask, capacity


def barcode_census_host(data, allowlist: Tuple[np.ndarray, np.ndarray] = _NO_LIST, hash_mask: Optional[int] = None,
                        initial_capacity: Optional[int] = None) -> BarcodeCensus:
    """`rocco_hip_barcode_census_host`: the census of all lines of host bytes on the calling thread, from the rules header the
    kernels compile, every array at its exact size (test support; no device is touched)."""
    out_bytes, offsets, records, lines, grows, capacity = barcode_census_host_arrays(data, allowlist, hash_mask, initial_capacity)
    return BarcodeCensus(out_bytes, offsets, records, lines, {"capacity": capacity, "grows": grows, "slabs": 1, "status": _native.OK})


def barcode_census_host_arrays(data, allowlist: Tuple[np.ndarray, np.ndarray] = _NO_LIST, hash_mask: Optional[int] = None,
                               initial_capacity: Optional[int] = None):
    """What `rocco_hip_barcode_census_host` writes, as it writes it: (the barcodes' bytes, the D + 1 offsets, the records -- in
    the order of the barcodes' first lines --, lines, grows, the capacity at the end)."""
    lib = _native.load()
    mask, capacity = _census_arguments(hash_mask, initial_capacity)
    raw = np.frombuffer(bytes(data), dtype=np.uint8).copy() if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    allow_bytes, allow_offsets = np.ascontiguousarray(allowlist[0], dtype=np.uint8), np.ascontiguousarray(allowlist[1], dtype=np.int64)
    n_allow = len(allow_offsets) - 1
    head = (raw.ctypes.data if raw.size else None, raw.size, allow_bytes.ctypes.data if allow_bytes.size else None,
            allow_offsets.ctypes.data if n_allow else None, n_allow, mask, capacity)
    report = (ctypes.c_longlong * 4)()
    _native.check(lib.rocco_hip_barcode_census_host(None, *head, None, 0, None, None, 0, report), "rocco_hip_barcode_census_host")
    entries, total = int(report[0]), int(report[1])
    out_bytes, offsets, records = np.empty(total, dtype=np.uint8), np.empty(entries + 1, dtype=np.int64), np.empty(entries, dtype=np.int64)
    _native.check(lib.rocco_hip_barcode_census_host(None, *head, out_bytes.ctypes.data if total else None, total, offsets.ctypes.data,
                                                    records.ctypes.data, entries, report), "rocco_hip_barcode_census_host")
    final = capacity
    while final < 2 * entries:
        final *= 2
    return out_bytes, offsets, records, int(report[2]), int(report[3]), final


class BarcodeCensusTable:
    """The device structure of the census: an open-addressing table of 64-bit slots with a 64-bit counter each, and an arena
    with the bytes, offsets and hashes of the barcodes settled so far, as CUDA tensors this object owns.  `insert` takes one
    slab (text in HBM and its line starts), `census` hands the result to the host.  Before a slab the table is grown by
    `rocco_hip_barcode_census_rehash` until it has twice as many slots as there are entries and lines of the slab together;
    with that bound every probe ends.  ``allowlist``: a packed, sorted list (`parse_barcode_allowlist`), applied per line."""

    def __init__(self, device=None, allowlist: Tuple[np.ndarray, np.ndarray] = _NO_LIST, hash_mask: Optional[int] = None,
                 initial_capacity: Optional[int] = None):
        import torch

        self.device = _dp._device(device)
        self.mask, self.capacity = _census_arguments(hash_mask, initial_capacity)
        self.entries = self.used = self.lines = self.grows = self.slabs = 0
        self.status = _native.OK
        self.n_allow = len(allowlist[1]) - 1
        with torch.cuda.device(self.device):
            self.allow_bytes = torch.from_numpy(np.ascontiguousarray(allowlist[0], dtype=np.uint8)).to(self.device)
            self.allow_offsets = torch.from_numpy(np.ascontiguousarray(allowlist[1], dtype=np.int64)).to(self.device)
            self.slots = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
            self.counts = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
            self.arena_bytes = torch.empty(0, dtype=torch.uint8, device=self.device)
            self.arena_offsets = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.arena_hashes = torch.empty(0, dtype=torch.int64, device=self.device)

    def _solver(self):
        return _native.solver_for(self.device.index).handle

    def _room(self, n_lines: int, n_bytes: int, stream) -> None:
        import torch

        need = self.entries + n_lines
        if self.capacity < 2 * need:
            capacity = self.capacity
            while capacity < 2 * need:
                capacity *= 2
            slots = torch.empty(capacity, dtype=torch.int64, device=self.device)
            counts = torch.empty(capacity, dtype=torch.int64, device=self.device)
            self.status = _native.load().rocco_hip_barcode_census_rehash(
                self._solver(), self.slots.data_ptr(), self.counts.data_ptr(), self.capacity, slots.data_ptr(), counts.data_ptr(), capacity,
                self.arena_hashes.data_ptr(), self.entries, self.mask, stream)
            _native.check(self.status, "rocco_hip_barcode_census_rehash")
            self.slots, self.counts, self.capacity, self.grows = slots, counts, capacity, self.grows + 1
        if int(self.arena_hashes.shape[0]) < max(need, 1):
            room = max(need, 1, 2 * int(self.arena_hashes.shape[0]))
            offsets = torch.zeros(room + 1, dtype=torch.int64, device=self.device)
            hashes = torch.empty(room, dtype=torch.int64, device=self.device)
            offsets[: self.entries + 1] = self.arena_offsets[: self.entries + 1]
            hashes[: self.entries] = self.arena_hashes[: self.entries]
            self.arena_offsets, self.arena_hashes = offsets, hashes
        if int(self.arena_bytes.shape[0]) < self.used + n_bytes:
            grown = torch.empty(max(self.used + n_bytes, 2 * int(self.arena_bytes.shape[0])), dtype=torch.uint8, device=self.device)
            grown[: self.used] = self.arena_bytes[: self.used]
            self.arena_bytes = grown

    def insert(self, bytes_t, starts_t, n_bytes: Optional[int] = None) -> Tuple[int, int]:
        """`rocco_hip_barcode_census_insert` of the lines ``starts_t`` (n_lines + 1 starts, as `lines_device` gives them) of the
        text ``bytes_t``: (new entries, the bytes they added to the arena).  The slab is not needed afterwards."""
        import torch

        if (not _dp._is_tensor(bytes_t) or bytes_t.dtype != torch.uint8 or bytes_t.dim() != 1 or bytes_t.device != self.device or
                not _dp._is_tensor(starts_t) or starts_t.dtype != torch.int64 or starts_t.dim() != 1 or starts_t.device != self.device or
                int(starts_t.shape[0]) < 1):
            raise TypeError("BarcodeCensusTable.insert: a uint8 tensor and the int64 tensor of its n_lines + 1 line starts, on the table's device, are required")
        bytes_t, starts_t = bytes_t.contiguous(), starts_t.contiguous()
        n = int(bytes_t.shape[0]) if n_bytes is None else int(n_bytes)
        n_lines = int(starts_t.shape[0]) - 1
        if not 0 <= n <= int(bytes_t.shape[0]):
            raise ValueError("BarcodeCensusTable.insert: n_bytes lies outside the tensor")
        report = (ctypes.c_longlong * 4)()
        with torch.cuda.device(self.device):
            stream = _dp._stream_ptr(bytes_t)
            self._room(n_lines, n, stream)
            self.status = _native.load().rocco_hip_barcode_census_insert(
                self._solver(), bytes_t.data_ptr(), n, starts_t.data_ptr(), n_lines, self.allow_bytes.data_ptr(), self.allow_offsets.data_ptr(),
                self.n_allow, self.slots.data_ptr(), self.counts.data_ptr(), self.capacity, self.arena_bytes.data_ptr(),
                int(self.arena_bytes.shape[0]), self.arena_offsets.data_ptr(), self.arena_hashes.data_ptr(), int(self.arena_hashes.shape[0]),
                self.entries, self.used, self.mask, report, stream)
            _native.check(self.status, "rocco_hip_barcode_census_insert")
        self.entries, self.used = self.entries + int(report[0]), self.used + int(report[1])
        self.lines, self.slabs = self.lines + n_lines, self.slabs + 1
        return int(report[0]), int(report[1])

    def census(self) -> BarcodeCensus:
        """`rocco_hip_barcode_census_records`, then the D entries go to the host and are put in order there."""
        import torch

        with torch.cuda.device(self.device):
            records = torch.zeros(self.entries, dtype=torch.int64, device=self.device)
            self.status = _native.load().rocco_hip_barcode_census_records(
                self._solver(), self.slots.data_ptr(), self.counts.data_ptr(), self.capacity, self.entries, records.data_ptr(),
                _dp._stream_ptr(self.slots))
            _native.check(self.status, "rocco_hip_barcode_census_records")
            return BarcodeCensus(self.arena_bytes[: self.used].cpu().numpy(), self.arena_offsets[: self.entries + 1].cpu().numpy(),
                                 records.cpu().numpy(), self.lines,
                                 {"capacity": self.capacity, "grows": self.grows, "slabs": self.slabs, "status": self.status})


def barcode_census_device(bytes_t, starts_t=None, allowlist: Tuple[np.ndarray, np.ndarray] = _NO_LIST, hash_mask: Optional[int] = None,
                          initial_capacity: Optional[int] = None, n_bytes: Optional[int] = None) -> BarcodeCensus:
    """The census of text that already lies in HBM: a one-dimensional uint8 CUDA tensor and, where the caller has them, its
    line starts (`lines_device` makes them otherwise).  Several slabs go through one `BarcodeCensusTable`."""
    if starts_t is None:
        starts_t, _ = lines_device(bytes_t, 0, n_bytes)
    table = BarcodeCensusTable(bytes_t.device, allowlist, hash_mask, initial_capacity)
    table.insert(bytes_t, starts_t, n_bytes)
    return table.census()


def barcode_census(source, device=None, inflate: Optional[str] = None, slab_bytes: int = DEFAULT_SLAB_BYTES, threads: Optional[int] = None,
                   hash_mask: Optional[int] = None, initial_capacity: Optional[int] = None) -> BarcodeCensus:
    """The distinct barcodes of the WHOLE fragments file ``source`` (a path or a `FragmentsSource`; its allow-list, where it
    has one, is applied per line) and the lines of each, in one pass on the device: the file goes through in slabs cut at
    BGZF block boundaries exactly as `get_fragments_mapped_read_count` walks it -- host or device inflate, the unfinished
    last line of a slab carried into the next --, every slab through the line pass and `BarcodeCensusTable.insert`.

    The rule of a line is ``ccounts_getCellCount``'s (ccounts_backend.c:1937-1975), not the field pass's: fields end at TAB,
    the scan of a line ends at LF, CR or NUL, the barcode is field 3; a line without one or with an empty one contributes
    nothing; a ``#`` line is a line like any other; an unterminated last line is read.  No other column is parsed, so the
    dialect errors of the field pass (`_ERROR_TEXT`) do NOT apply to this call: a file the count refuses has a census.
    ``hash_mask`` (ANDed with every hash; the result never depends on it) and ``initial_capacity`` are for tests."""
    import torch

    source = _as_source(source)
    inflate = _bam.DEFAULT_INFLATE if inflate is None else inflate
    if inflate not in ("host", "device"):
        raise ValueError(f"barcode_census: inflate must be \"host\" or \"device\", not {inflate!r}")
    dev = _dp._device(device)
    table, carry = BarcodeCensusTable(dev, source.allowlist(), hash_mask, initial_capacity), None
    with torch.cuda.device(dev):
        slabs = iter(_whole_file_slabs(source, dev, inflate, max(1, int(slab_bytes)), threads))
        slab = next(slabs, None)
        while slab is not None:
            following = next(slabs, None)
            data = slab if carry is None or not int(carry.shape[0]) else torch.cat([carry, slab])
            n, carry = int(data.shape[0]), None
            starts, report = lines_device(data)
            n_lines = report["lines"]
            if following is not None and report["open"]:
                n_lines, n = n_lines - 1, report["cut"]
                starts, carry = starts[: n_lines + 1], data[n:].clone()
            if n_lines:
                table.insert(data, starts, n_bytes=n)
            slab = following
    return table.census()


def get_fragments_cell_count(source, device=None, inflate: Optional[str] = None, slab_bytes: int = DEFAULT_SLAB_BYTES,
                             threads: Optional[int] = None) -> int:
    """``ccounts_getCellCount`` (ccounts_backend.c:1890-2046): the number of distinct barcodes of a fragments file under the
    source's allow-list, ``len(barcode_census(...))``.  The index is opened first, as the reference opens the source with it
    (RuntimeError with the reference's words for a file without one); a ``.bam`` path is the reference's RuntimeError "cell
    count is only supported for fragments sources"."""
    source = _as_source(source)
    if source.path.lower().endswith(".bam"):
        raise RuntimeError("cell count is only supported for fragments sources")
    _index_of(source)
    return len(barcode_census(source, device=device, inflate=inflate, slab_bytes=slab_bytes, threads=threads))


def get_fragments_read_length(source, min_reads: int = 32, max_iterations: int = 4096) -> int:
    """``ccounts_getReadLength`` over a fragments source (687-779), on the host from the file's leading blocks: the median of
    the fragment lengths of the first ``min(min_reads, max_iterations)`` valid lines (three fields, both integers parse,
    end > start; an even count gives the floor of the mean of the two middle values in uint32).  RuntimeError with the
    reference's words where the file has no valid line.  Needs no index."""
    source = _as_source(source)
    min_reads, max_iterations = int(min_reads), int(max_iterations)
    if min_reads <= 0:  # (ccounts_backend.c:676-685: the reference's defaults for what is not positive)
        min_reads = 1
    if max_iterations < min_reads:
        max_iterations = min_reads
    want = min(min_reads, max_iterations)
    raw = _bam._mapped_bytes(source.path)
    blocks = _bam._bgzf_blocks(raw, source.path)
    text, taken, lengths = b"", 0, np.zeros(0, dtype=np.int64)
    while True:
        upto = min(len(blocks), max(2 * taken, 4))
        text += b"".join(_bam._inflate_block(raw, source.path, k, blocks[k]) for k in range(taken, upto))
        taken = upto
        whole = taken == len(blocks)
        usable = text if whole else text[: text.rfind(b"\n") + 1]
        if usable:
            got = fragfile_host(usable, whole_file=True)
            if got["report"][0] >= 0:
                valid_before = _valid_read_length(got, got["report"][0])
                if valid_before.size < want:  # (the reference would have read this line: it is refused, not skipped)
                    raise ValueError(f"{source.path}: line {got['report'][0] + 1} of the file: {_ERROR_TEXT.get(got['report'][1], 'error')}")
                lengths = valid_before
            else:
                lengths = _valid_read_length(got, got["lines"])
        if lengths.size >= want or whole:
            break
    lengths = np.sort(lengths[:want].astype(np.uint32))
    if lengths.size == 0:
        raise RuntimeError("failed to estimate fragment length from fragments source")
    mid = lengths.size // 2
    if lengths.size % 2 == 0:
        return int((np.uint32(lengths[mid - 1]) + np.uint32(lengths[mid])) // np.uint32(2))  # (the sum wraps in uint32, as the reference's does)
    return int(lengths[mid])


def _valid_read_length(got: dict, upto: int) -> np.ndarray:
    status, start, end = got["status"][:upto], got["start"][:upto].astype(np.int64), got["end"][:upto].astype(np.int64)
    ok = ((status & START_OK) != 0) & ((status & END_OK) != 0) & (end > start)
    return (end - start)[ok]


# --------------------------------------------------------------------------------------------
# the Python level: metadata, one chromosome of one source, K sources -> the count matrix
# --------------------------------------------------------------------------------------------

_FRAGMENTS_COUNT_METADATA_CACHE: dict = {}


def _source_name(source) -> str:
    return _as_source(source).path


def _get_fragments_count_metadata(source, step: int, norm_method: str, effective_genome_size: float, ignore_for_norm, flag_exclude: int = 0,
                                  extend_reads: int = -1, num_processors: int = 1, scale_factor: float = 1.0) -> dict:
    """rocco/readtracks.py:242-353 with the fragments answers of the backend: the source is never paired-end
    (ccounts_backend.c:614-617), the read length is `get_fragments_read_length`, the mapped count is
    `get_fragments_mapped_read_count` under ``coverage``; ``extend_reads == 0`` asks for a fragment-length estimate, which
    the backend refuses for this source ("source kind is not BAM", 968-971).  Flags have no effect."""
    source = _as_source(source)
    ignore = tuple(ignore_for_norm or [])
    threads = _bam._resolve_num_processors(num_processors)
    cache_key = (source.path, source.barcode_allowlist_file, int(step), _bam._clean_string(norm_method).upper(),
                 float(effective_genome_size if effective_genome_size is not None else -1.0), ignore, int(flag_exclude), int(extend_reads),
                 int(threads), float(scale_factor))
    if cache_key in _FRAGMENTS_COUNT_METADATA_CACHE:
        return _FRAGMENTS_COUNT_METADATA_CACHE[cache_key]
    paired_end = False
    read_length = int(get_fragments_read_length(source, min_reads=32, max_iterations=4096))
    mapped_reads, _ = get_fragments_mapped_read_count(source, list(ignore), "coverage", 0)
    norm_read_length, resolved_extend_bp = int(read_length), int(extend_reads)
    if int(extend_reads) == 0:
        raise RuntimeError("source kind is not BAM")
    if int(extend_reads) > 0:
        norm_read_length = resolved_extend_bp = int(extend_reads)
    norm_scale = _rt._compute_native_scale_factor(norm_method, effective_genome_size, step, int(mapped_reads), int(norm_read_length),
                                                  float(scale_factor))
    metadata = {"paired_end": paired_end, "paired_end_mode": False, "read_length": int(read_length), "norm_read_length": int(norm_read_length),
                "resolved_extend_bp": int(resolved_extend_bp), "mapped_reads": int(mapped_reads), "norm_scale": float(norm_scale),
                "threads": int(threads)}
    _FRAGMENTS_COUNT_METADATA_CACHE[cache_key] = metadata
    return metadata


def _chrom_reads_batch(sources: List[FragmentsSource], chromosome: str, chrom_size: int, step: int, metadata_list, center_reads: bool,
                       const_scale: float, round_digits: int, scale_by_step: bool, count_mode: str, device=None, inflate=None):
    """rocco/readtracks.py:439-518 for K sources of one chromosome: the ranges of all K in one call, the counts in one launch
    series, the tail per source.  Returns (intervals, values) lists with None for a source without data."""
    K = len(sources)
    intervals_out, vals_out = [None] * K, [None] * K
    lines = read_fragments_spans([(s, chromosome) for s in sources], device=device, inflate=inflate)
    known = [k for k in range(K) if lines[k] is not None]
    ranges = dict(zip(known, chrom_ranges_batch_device([lines[k] for k in known], [chrom_size] * len(known)))) if known else {}
    # the reference works file by file, so its log records come file by file: what the sources log while they are worked
    # on together is held and handed on afterwards in the reference's order (as `rocco_amd.bam.generate_chrom_matrix_device` does)
    live, regions, logged = [], [], [[] for _ in range(K)]
    held = _bam._HeldRecords()
    logger.addFilter(held)
    try:
        for k in range(K):
            chrom_start, chrom_end = ranges.get(k, (0, 0))
            if chrom_end <= chrom_start:
                logger.warning("No mapped reads found in BAM file: %s for chromosome: %s. Returning (None,None).", sources[k].path, chromosome)
                logged[k], held.records = held.records, []
                continue
            live.append(k)
            regions.append(_rt._count_window(chrom_start, chrom_end, chrom_size, step) + (step,))
        if live:
            mode = parse_count_mode(count_mode)
            counts, _ = count_lines_batch_device([lines[k] for k in live], regions, [mode] * len(live), [1 if center_reads else 0] * len(live))
            for k, region, counted in zip(live, regions, counts):
                intervals_out[k], vals_out[k] = _rt._bam_tail(counted, region[0], step, float(metadata_list[k]["norm_scale"]), scale_by_step,
                                                              const_scale, round_digits, sources[k].path, chromosome)
                logged[k], held.records = held.records, []
    finally:
        logger.removeFilter(held)
        for record in [r for records in logged for r in records] + held.records:
            logger.handle(record)  # (also where an error cut the call short: what was logged up to it is not lost)
    return intervals_out, vals_out


def _front_checks(source: FragmentsSource, chromosome: str, chrom_sizes_file: str) -> int:
    if not os.path.exists(source.path):
        raise FileNotFoundError(f"BAM file not found: {source.path}")
    if not os.path.exists(chrom_sizes_file):
        raise FileNotFoundError(f"Chromosome sizes file not found: {chrom_sizes_file}")
    sizes = _rt.get_chroms_and_sizes(chrom_sizes_file)
    if chromosome not in sizes:
        raise ValueError(f"Chromosome {chromosome} not found in chromosome sizes file: {chrom_sizes_file}")
    return int(sizes[chromosome])


def get_fragments_chrom_reads(source, chromosome: str, chrom_sizes_file: str, step: int, effective_genome_size: float = -1,
                              norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                              extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                              num_processors: int = -1, const_scale: float = 1.0, round_digits: int = 5, scale_by_step: bool = False,
                              count_mode: str = "coverage"):
    """The reference's ``get_bam_chrom_reads`` (rocco/readtracks.py:389-518; same keywords, return value, errors and warnings)
    over a fragments source, plus ``count_mode``.  Flags and the mapping quality have no effect on this source.  The tail
    (scaling in float64, the positive support, np.round) is `rocco_hip_alignment_count_tail_f64`."""
    source = _as_source(source)
    chrom_size = _front_checks(source, chromosome, chrom_sizes_file)
    parse_count_mode(count_mode)
    if ignore_for_norm is None:
        ignore_for_norm = ["chrX", "chrY", "chrM"]
    metadata = _get_fragments_count_metadata(source, step=step, norm_method=norm_method, effective_genome_size=effective_genome_size,
                                             ignore_for_norm=ignore_for_norm, flag_exclude=flag_exclude, extend_reads=extend_reads,
                                             num_processors=num_processors, scale_factor=scale_factor)
    intervals, vals = _chrom_reads_batch([source], chromosome, chrom_size, int(step), [metadata], center_reads, const_scale, round_digits,
                                         scale_by_step, count_mode)
    return intervals[0], vals[0]


def generate_chrom_matrix_device(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, const_scale: float = 1.0,
                                 round_digits: int = 5, scale_by_step: bool = False, effective_genome_size: float = -1,
                                 norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                                 extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                                 num_processors: int = -1, low_memory: bool = False, count_mode: str = "coverage"):
    """The reference's ``generate_chrom_matrix`` (rocco/readtracks.py:521-633, same keywords plus ``count_mode``) over K
    fragments sources (paths or `FragmentsSource`s: one file with K allow-lists gives a K-row pseudo-bulk matrix) with the
    matrix left on the device: (starts as a host ``int`` array, count matrix as a CUDA tensor), or ``(None, None)``.  Per
    source, in order, the checks and the metadata of `get_fragments_chrom_reads`; then the ranges of all K in one call, the
    counts in one launch series and the existing assembly.  This is the function to bind behind
    ``rocco_amd.rocco.generate_chrom_matrix``."""
    sources = [_as_source(f) for f in input_files]
    parse_count_mode(count_mode)
    if ignore_for_norm is None:
        ignore_for_norm = ["chrX", "chrY", "chrM"]
    metadata_list, chrom_size = [], 0
    for source in sources:
        chrom_size = _front_checks(source, chromosome, chrom_sizes_file)
        metadata_list.append(_get_fragments_count_metadata(source, step=step, norm_method=norm_method, effective_genome_size=effective_genome_size,
                                                           ignore_for_norm=ignore_for_norm, flag_exclude=flag_exclude, extend_reads=extend_reads,
                                                           num_processors=num_processors, scale_factor=scale_factor))
    intervals, vals = _chrom_reads_batch(sources, chromosome, chrom_size, int(step), metadata_list, center_reads, const_scale, round_digits,
                                         scale_by_step, count_mode)
    has_data = [i is not None and v is not None for i, v in zip(intervals, vals)]
    _rt._emit(_rt._excluded_records([s.path for s in sources], has_data, chromosome))
    if not any(has_data):
        return None, None
    common, matrix = _rt.assemble_chrom_matrix_device([i for i in intervals if i is not None], [v for v in vals if v is not None],
                                                      track_type="bam", low_memory=low_memory, chromosome=chromosome)
    return common.cpu().numpy().astype(int), matrix


def generate_chrom_matrix(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, *args, **kwargs):
    """`generate_chrom_matrix_device` with the reference's return value: NumPy ``(common_intervals.astype(int), count_matrix)``,
    or ``(None, None)``."""
    starts, matrix = generate_chrom_matrix_device(chromosome, input_files, chrom_sizes_file, step, *args, **kwargs)
    if starts is None:
        return None, None
    return starts, matrix.cpu().numpy()
