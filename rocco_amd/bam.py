"""Read BAM files (note (29)): BGZF blocks are inflated on the host with Python's zlib (the default)
or on the device (``inflate="device"``: csrc/bgzf_inflate.hip, DEFLATE and CRC32 in HIP, one wavefront per block), everything
after the inflate runs on the device (csrc/bam_records.hip): the record walk over the inflated bytes, the seven values per
record that rows f5-f7 consume, and the split by contig.  Both modes share one front (the file read once, `_bgzf_blocks`, the
slab rule `_slab_groups`, one wording of the block errors) and one loop in `read_alignment_file`, which takes the header
first and then slabs of inflated bytes as device tensors, wherever they were inflated.  `get_bam_chrom_reads` and `_get_bam_count_metadata` have the
reference's signatures (rocco/readtracks.py:389-407, 242-252) and are composed from `read_alignment_file`,
`rocco_amd.readtracks.bam_count_metadata_from_records` and `bam_chrom_reads_from_records`; an integrator binds the first
behind the stub: ``rocco_amd.readtracks.get_bam_chrom_reads = rocco_amd.bam.get_bam_chrom_reads``.

A file that has a ``.bai`` index (rocco_amd/bam_index.py) is read contig by contig (note (32)):
`read_alignment_spans` lays the spans of K (file, contig) pairs one behind the other -- with the index each begins and ends on
a record boundary, so they form one record chain -- and decodes a group of them with one inflate, one walk and one field
decode; `rocco_hip_bam_stream_firsts` splits the chain back and checks what the index claimed.  `_cached_file` hands out an
`IndexedAlignmentFile` for such a file (``USE_INDEX``), which decodes a contig when it is asked for.

Not built: CRAM and SAM, ``.csi`` indexes (such a file is decoded whole; the index iterator's overlap test is already applied
by the counting kernels), CIGARs kept in a ``CG`` tag (reported as an error).  There is no CPU fallback for the record walk."""
from __future__ import annotations

import bisect
import collections
import collections.abc
import ctypes
import logging
import multiprocessing
import os
import struct
import zlib
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import _native
from . import bam_index as _bai
from . import dp as _dp
from . import readtracks as _rt
from .inflate import (  # noqa: F401  (what the bigWig reader shares; the names stay importable from here)
    BGZF_ERR_CRC, BGZF_ERR_LENGTH, BGZF_ERR_STREAM, BGZF_ERR_TABLE, BGZF_MAX_GRID, BGZF_MAX_ISIZE, BGZF_STREAM_REASONS, BGZF_TABLE_COLUMNS,
    BGZF_THREADS, _STREAM_REASON_TEXT, SpanList, _default_threads, _host_buffer, bgzf_block_table, bgzf_shape, inflate_blocks_device,
    inflate_blocks_host, on_pool, refuse_large_blocks, upload_blocks)
from .readtracks import AlignmentFileRecords, AlignmentRecords

logger = _rt.logger  # (the reference's reader logs where its readtracks module does)

DEFAULT_SLAB_BYTES = 256 << 20
DEFAULT_BATCH_BYTES = 2 << 30  # inflated bytes of one group of `read_alignment_spans` (a choice, not a measurement: DESIGN.md note (32))
USE_INDEX = True               # `_cached_file` reads a file that has a .bai index contig by contig (rocco_amd/bam_index.py)
DEFAULT_INFLATE = "host"       # where `get_bam_chrom_reads` and `_get_bam_count_metadata` have a file's blocks inflated: "host" or "device"
GUESS_DEPTH = 3                # ROCCO_BAM_GUESS_DEPTH of include/rocco_hip.h
DEFAULT_SEGMENT_BYTES = 16384  # ROCCO_BAM_SEGMENT_BYTES
_BGZF_HEADER = 12              # ID1 ID2 CM FLG MTIME(4) XFL OS XLEN(2)

ERR_BLOCK_SIZE, ERR_TRUNCATED, ERR_SIZES, ERR_READ_NAME, ERR_REF_ID, ERR_CIGAR_SEQ, ERR_POSITION, ERR_END, ERR_CG_TAG, ERR_ORDER, \
    ERR_OFFSET = range(1, 12)
ERR_SEAM, ERR_SPAN_TID = 12, 13  # (of `rocco_hip_bam_stream_firsts`: what an index that does not describe its file looks like)
_ERROR_TEXT = {
    ERR_BLOCK_SIZE: "its block_size is below 32",
    ERR_TRUNCATED: "the stream ends inside it",
    ERR_SIZES: "its name, CIGAR, sequence and qualities do not fit its block_size",
    ERR_READ_NAME: "its l_read_name is 0",
    ERR_REF_ID: "its refID or next_refID is outside the header's contigs",
    ERR_CIGAR_SEQ: "the query length of its CIGAR differs from l_seq",
    ERR_POSITION: "it lies on a contig at a negative position",
    ERR_END: "it ends at or beyond 2**31",
    ERR_CG_TAG: "its first CIGAR operation soft-clips the whole sequence: the real CIGAR may be kept in a CG tag, which is not decoded",
    ERR_ORDER: "its contig comes before the previous record's: the file is not coordinate-sorted (contigs in header order, "
               "records without a contig last)",
    ERR_OFFSET: "no record is framed there",
}


# --------------------------------------------------------------------------------------------
# BGZF: the front both inflates share (source, blocks, slab rule, error words) and the host inflate
# --------------------------------------------------------------------------------------------

def _source_bytes(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return memoryview(source), "<bytes>"
    with open(os.fspath(source), "rb") as handle:
        return memoryview(handle.read()), os.fspath(source)


def _block_where(name: str, index: int, at: int) -> str:
    return f"{name}: BGZF block {index} at file offset {at}"


def _does_not_inflate(where: str, why: str) -> ValueError:
    return ValueError(f"{where}: the deflate stream does not inflate ({why})")


def _length_mismatch(where: str, isize: int, produced: int) -> ValueError:
    return ValueError(f"{where}: length mismatch (ISIZE says {isize}, the data inflates to {produced})")


def _crc_mismatch(where: str) -> ValueError:
    return ValueError(f"{where}: CRC32 mismatch")


def _bgzf_block_at(raw, total: int, at: int, bad) -> Tuple[int, int, int, int, int]:
    """The row of the block whose header begins at file offset ``at``; ``bad(what)`` makes the error for a header that is refused."""
    if at + _BGZF_HEADER > total:
        raise bad("the file ends inside the block header")
    id1, id2, cm, flg = raw[at], raw[at + 1], raw[at + 2], raw[at + 3]
    if id1 != 0x1F or id2 != 0x8B or cm != 8:
        raise bad("bad header (no gzip magic)")
    if not flg & 4:
        raise bad("bad header (FLG.FEXTRA is not set)")
    (xlen,) = struct.unpack_from("<H", raw, at + 10)
    extra, extra_end = at + _BGZF_HEADER, at + _BGZF_HEADER + xlen
    if extra_end > total:
        raise bad("the file ends inside the block header")
    bsize = None
    while extra + 4 <= extra_end:
        si1, si2, slen = raw[extra], raw[extra + 1], struct.unpack_from("<H", raw, extra + 2)[0]
        if extra + 4 + slen > extra_end:
            raise bad("bad header (an extra subfield overruns XLEN)")
        if si1 == 66 and si2 == 67 and slen == 2:
            bsize = struct.unpack_from("<H", raw, extra + 4)[0] + 1
        extra += 4 + slen
    if bsize is None:
        raise bad("bad header (no BC subfield)")
    if bsize < _BGZF_HEADER + xlen + 8:
        raise bad("bad header (BSIZE is smaller than the header and trailer)")
    if at + bsize > total:
        raise bad(f"the file ends inside the block ({total - at} of {bsize} bytes)")
    crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
    return at, extra_end, at + bsize - 8, crc, isize


def _bgzf_blocks(raw: memoryview, name: str) -> List[Tuple[int, int, int, int, int]]:
    """(file offset, first byte of the deflate data, one past its last, CRC32, ISIZE) per block, from the block headers."""
    blocks, at, total = [], 0, len(raw)

    def bad(what: str) -> ValueError:  # (worded only where a block is refused: a file has tens of thousands of blocks)
        return ValueError(f"{_block_where(name, len(blocks), at)}: {what}")

    while at < total:
        block = _bgzf_block_at(raw, total, at, bad)
        blocks.append(block)
        at = block[2] + 8
    return blocks


def _bgzf_span_blocks(raw, name: str, contig: str, v_begin: int, v_end: int):
    """The ranged front: (the block rows from file offset ``v_begin >> 16`` up to and including the block at ``v_end >> 16``
    -- left out where ``v_end & 0xFFFF == 0`` --, the bytes to skip in the first block, the bytes to keep of the last).  The
    checks and words of `_bgzf_blocks`; the blocks are numbered from the span's first.  ``skip == ISIZE`` is legal (htslib may
    point at a block's end: such a block contributes nothing).  ValueError naming the file, the contig and the virtual offset
    for a span that points outside the file or past a block's ISIZE."""
    total = len(raw)
    first, skip, last, keep = int(v_begin) >> 16, int(v_begin) & 0xFFFF, int(v_end) >> 16, int(v_end) & 0xFFFF

    def outside(v: int, why: str) -> ValueError:
        return ValueError(f"{name}: contig {contig}: virtual offset {v} ({v >> 16} << 16 | {v & 0xFFFF}) of the index {why}")

    if v_end < v_begin:
        raise outside(v_end, f"ends the span before its begin, virtual offset {v_begin}")
    blocks, at = [], first

    def bad(what: str) -> ValueError:
        return ValueError(f"{_block_where(name, len(blocks), at)} (blocks counted from the span of contig {contig}): {what}")

    while at < last or (at == last and keep != 0):
        if at >= total:
            raise outside(v_end if blocks else v_begin, f"points outside the file ({total} bytes)")
        block = _bgzf_block_at(raw, total, at, bad)
        blocks.append(block)
        at = block[2] + 8
    if (keep != 0 and blocks[-1][0] != last) or (keep == 0 and at != last):
        raise outside(v_end, f"names no block: the blocks from the span's begin pass it, the next begins at file offset {at}")
    if keep == 0:
        keep = blocks[-1][4] if blocks else 0
    if blocks and skip > blocks[0][4]:
        raise outside(v_begin, f"points past the block's ISIZE ({blocks[0][4]})")
    if blocks and keep > blocks[-1][4]:
        raise outside(v_end, f"points past the block's ISIZE ({blocks[-1][4]})")
    return blocks, skip, keep


def _bgzf_front(source, slab_bytes: Optional[int], who: str):
    """What both inflates start from: (the source's bytes, read once; its name; its blocks, walked once; ``slab_bytes`` checked)."""
    if slab_bytes is not None and int(slab_bytes) < 1:
        raise ValueError(f"{who}: slab_bytes must be positive")
    raw, name = _source_bytes(source)
    return raw, name, _bgzf_blocks(raw, name), None if slab_bytes is None else int(slab_bytes)


def _slab_groups(blocks, slab_bytes: Optional[int]):
    """(first, one past the last) block of every slab: a slab holds at least ``slab_bytes`` inflated bytes (everything for
    None) and at least one block; trailing empty blocks go with the slab before."""
    first = 0
    while first < len(blocks):
        last, size = first, 0
        while last < len(blocks) and (slab_bytes is None or size < slab_bytes or last == first):
            size += blocks[last][4]
            last += 1
        while last < len(blocks) and blocks[last][4] == 0:  # (the end-of-file marker and its like)
            last += 1
        yield first, last
        first = last


def _whole_or_slabs(slabs, slab_bytes: Optional[int], empty):
    """The generator itself where slabs were asked for, else the one slab of the whole stream (``empty()`` for no block)."""
    if slab_bytes is not None:
        return slabs
    slabs = list(slabs)
    return slabs[0] if slabs else empty()


def _inflate_block(raw: memoryview, name: str, index: int, block) -> bytes:
    """One block through zlib, its length and CRC32 checked."""
    at, lo, hi, crc, isize = block
    where = _block_where(name, index, at)
    try:
        data = zlib.decompress(raw[lo:hi], wbits=-15)
    except zlib.error as exc:
        raise _does_not_inflate(where, exc) from None
    if len(data) != isize:
        raise _length_mismatch(where, isize, len(data))
    if zlib.crc32(data) != crc:
        raise _crc_mismatch(where)
    return data


def _inflate_slabs(raw: memoryview, name: str, blocks, threads: Optional[int], slab_bytes: Optional[int]) -> Iterator[np.ndarray]:
    for first, last in _slab_groups(blocks, slab_bytes):
        starts = np.zeros(last - first + 1, dtype=np.int64)
        np.cumsum([b[4] for b in blocks[first:last]], out=starts[1:])
        out = _host_buffer(int(starts[-1]))

        def one(k):
            out[starts[k - first]: starts[k - first + 1]] = np.frombuffer(_inflate_block(raw, name, k, blocks[k]), dtype=np.uint8)

        on_pool(one, range(first, last), threads)
        yield out


def inflate_bgzf(source, threads: Optional[int] = None, slab_bytes: Optional[int] = None):
    """The inflated bytes of a BGZF file (``source``: a path or bytes) as a uint8 array in pinned host memory: the block
    headers are walked (gzip magic, FLG.FEXTRA, the ``BC`` subfield among possibly several, ``BSIZE``; ``CRC32`` and
    ``ISIZE`` from the trailer), the blocks are inflated with ``zlib.decompress(..., wbits=-15)`` on a pool of ``threads``
    threads (zlib releases the GIL; default ``min(16, len(os.sched_getaffinity(0)))``) and placed at the prefix sum of their
    ``ISIZE``; every block's length and CRC32 are checked.  ValueError naming the block and its file offset for a bad header,
    a mismatch or a file that ends inside a block; a missing end-of-file marker block is accepted.

    With ``slab_bytes``: a generator of such arrays, each of about that many inflated bytes (at least one block), cut at
    BGZF block boundaries (`_slab_groups`).  The block headers are walked, and their errors raised, at the call; a block is
    inflated and checked when its slab is asked for."""
    raw, name, blocks, slab_bytes = _bgzf_front(source, slab_bytes, "inflate_bgzf")
    return _whole_or_slabs(_inflate_slabs(raw, name, blocks, threads, slab_bytes), slab_bytes, lambda: _host_buffer(0))


# --------------------------------------------------------------------------------------------
# device: BGZF (csrc/bgzf_inflate.hip, csrc/inflate_core.h)
# --------------------------------------------------------------------------------------------

def _bgzf_error(where: str, isize: int, report: dict) -> ValueError:
    """The host path's words (`_inflate_block`) for a block the device refused."""
    code, why = report["status"] & 0xFF, report["status"] >> 8
    if code == BGZF_ERR_STREAM:
        return _does_not_inflate(where, _STREAM_REASON_TEXT.get(why, f"reason {why}"))
    if code == BGZF_ERR_LENGTH:
        return _length_mismatch(where, isize, report["produced"])
    if code == BGZF_ERR_CRC:
        return _crc_mismatch(where)
    return ValueError(f"{where}: its row of the block table does not fit the buffers (status {report['status']})")


def _inflate_slabs_device(raw: memoryview, name: str, blocks, dev, slab_bytes: Optional[int]):
    import torch

    refuse_large_blocks(blocks, lambda index, block: _block_where(name, index, block[0]))
    for first, last in _slab_groups(blocks, slab_bytes):
        group = blocks[first:last]
        base, end = group[0][1], group[-1][2]  # (a slab's blocks lie one behind the other: one span, headers and trailers ride along)
        table = bgzf_block_table(group, base)
        spans = SpanList()
        spans.add(raw, base, end)
        with torch.cuda.device(dev):
            table_t, comp_t = upload_blocks(table, spans.spans, spans.n_comp, dev)
            out = torch.empty(int(table[-1, 2] + table[-1, 4]), dtype=torch.uint8, device=dev)
            _, report = inflate_blocks_device(comp_t, table_t, out)  # (synchronises: the upload's pinned buffer may go)
        if report["block"] >= 0:
            bad = group[report["block"]]
            raise _bgzf_error(_block_where(name, first + report["block"], bad[0]), bad[4], report)
        yield out


def inflate_bgzf_device(source, device=None, slab_bytes: Optional[int] = None):
    """The device twin of `inflate_bgzf`: the inflated bytes of a BGZF file (``source``: a path or bytes) as a uint8 CUDA
    tensor.  The block headers are walked on the host as there; the compressed bytes go up from pinned memory with the block
    table, `rocco_hip_bgzf_inflate` inflates every block with one wavefront and checks its length and CRC32 on the device.
    The same ValueErrors as the host path, naming the block and its file offset (between the parentheses of ``the deflate
    stream does not inflate (...)`` stands the kernel's reason, in zlib's words); a block whose ISIZE exceeds 65 536 is
    refused.

    With ``slab_bytes``: a generator of such tensors, cut at BGZF block boundaries by the rule of `inflate_bgzf`."""
    import torch

    dev = _dp._device(device)
    raw, name, blocks, slab_bytes = _bgzf_front(source, slab_bytes, "inflate_bgzf_device")
    return _whole_or_slabs(_inflate_slabs_device(raw, name, blocks, dev, slab_bytes), slab_bytes,
                           lambda: torch.empty(0, dtype=torch.uint8, device=dev))


def _uploaded(slabs, dev):
    """Host slabs as device tensors, each uploaded asynchronously from its pinned array."""
    import torch

    for slab in slabs:
        up = torch.from_numpy(slab).to(dev, non_blocking=True)
        copied = torch.cuda.current_stream(dev).record_event()
        yield up
        copied.synchronize()  # (the pinned `slab` outlives its upload: it stays bound here until the copy has run)


def _header_from_leading_blocks(raw: memoryview, name: str, blocks):
    """(contigs, the offset of the first record) from a host inflate, into ordinary memory, of as many leading blocks as the
    header covers."""
    head, k = b"", 0
    while True:
        try:
            _, contigs, entry0 = parse_bam_header(head)
            return contigs, entry0
        except _HeaderCutShort as exc:
            if k == len(blocks):
                raise ValueError(f"{name}: {exc}") from None
        except ValueError as exc:
            raise ValueError(f"{name}: {exc}") from None
        head += _inflate_block(raw, name, k, blocks[k])
        k += 1


# --------------------------------------------------------------------------------------------
# host: the BAM header
# --------------------------------------------------------------------------------------------

class _HeaderCutShort(ValueError):
    """The bytes end inside the header (more of the stream may follow)."""


def parse_bam_header(inflated) -> Tuple[str, List[Tuple[str, int]], int]:
    """(text, [(name, length)] in header order, the byte offset of the first record) from the head of an inflated BAM stream:
    the magic ``BAM\\1``, ``l_text``, the text, ``n_ref`` and per contig ``l_name``, the NUL-terminated name and ``l_ref``.
    ValueError for anything else."""
    data = memoryview(np.ascontiguousarray(np.frombuffer(inflated, dtype=np.uint8) if not isinstance(inflated, np.ndarray) else inflated))
    total = len(data)

    def need(at, n, what):
        if at + n > total:
            raise _HeaderCutShort(f"BAM header: the stream ends inside {what} (at byte {at} of {total})")

    need(0, 4, "the magic")
    if bytes(data[0:4]) != b"BAM\x01":
        raise ValueError("BAM header: the magic is not `BAM\\1` (not a BAM file, or not inflated)")
    need(4, 4, "l_text")
    (l_text,) = struct.unpack_from("<i", data, 4)
    if l_text < 0:
        raise ValueError(f"BAM header: l_text is negative ({l_text})")
    need(8, l_text, "the text")
    text = bytes(data[8: 8 + l_text]).split(b"\0", 1)[0].decode("utf-8", "replace")
    at = 8 + l_text
    need(at, 4, "n_ref")
    (n_ref,) = struct.unpack_from("<i", data, at)
    if n_ref < 0:
        raise ValueError(f"BAM header: n_ref is negative ({n_ref})")
    at += 4
    contigs = []
    for k in range(n_ref):
        need(at, 4, f"l_name of contig {k}")
        (l_name,) = struct.unpack_from("<i", data, at)
        if l_name < 1:
            raise ValueError(f"BAM header: l_name of contig {k} is {l_name}")
        need(at + 4, l_name + 4, f"contig {k}")
        name = bytes(data[at + 4: at + 4 + l_name])
        if name[-1:] != b"\0":
            raise ValueError(f"BAM header: the name of contig {k} is not NUL-terminated")
        (l_ref,) = struct.unpack_from("<i", data, at + 4 + l_name)
        if l_ref < 0:
            raise ValueError(f"BAM header: the length of contig {k} is negative ({l_ref})")
        contigs.append((name[:-1].decode("utf-8", "replace"), int(l_ref)))
        at += 8 + l_name
    return text, contigs, at


# --------------------------------------------------------------------------------------------
# device: the record walk and the record fields (csrc/bam_records.hip)
# --------------------------------------------------------------------------------------------

def bam_shape() -> dict:
    """`rocco_hip_bam_shape`: the depth of a guess, the default segment size, the threads of a workgroup."""
    shape = (ctypes.c_int * 3)()
    _native.load().rocco_hip_bam_shape(shape)
    return {"guess_depth": int(shape[0]), "segment_bytes": int(shape[1]), "threads": int(shape[2])}


def walk_records_device(bytes_t, entry0: int, n_ref: int, segment_bytes: Optional[int] = None, guess_mode: int = 1,
                        want_segment_entries: bool = False):
    """`rocco_hip_bam_walk_records` over a uint8 CUDA tensor: (int64 CUDA tensor of the record offsets in stream order, report).
    The report: ``records``, ``end_offset`` (behind the last complete record), ``segments``, ``wrong_guesses``,
    ``repair_rounds`` (segments walked again), ``error`` (0, ERR_BLOCK_SIZE or ERR_TRUNCATED) and ``error_offset``; with
    ``want_segment_entries`` also ``segment_entries``, the confirmed entry of every segment or -1."""
    import torch

    lib = _native.load()
    if not _dp._is_tensor(bytes_t) or bytes_t.dtype != torch.uint8 or bytes_t.dim() != 1 or not bytes_t.is_cuda:
        raise TypeError("walk_records_device: a one-dimensional uint8 CUDA tensor is required")
    bytes_t = bytes_t.contiguous()
    n_bytes = int(bytes_t.shape[0])
    S = DEFAULT_SEGMENT_BYTES if segment_bytes is None else int(segment_bytes)
    capacity = n_bytes // 36 + 1
    offsets = torch.empty(capacity, dtype=torch.int64, device=bytes_t.device)
    segments = max((n_bytes + S - 1) // S, 1) if S > 0 else 1
    entries = torch.empty(segments, dtype=torch.int64, device=bytes_t.device) if want_segment_entries else None
    back = (ctypes.c_longlong * 8)()
    _native.check(lib.rocco_hip_bam_walk_records(
        _native.solver_for(bytes_t.device.index).handle, bytes_t.data_ptr(), n_bytes, int(entry0), int(n_ref), S, int(guess_mode),
        offsets.data_ptr(), capacity, entries.data_ptr() if entries is not None else None, back, _dp._stream_ptr(bytes_t)),
        "rocco_hip_bam_walk_records")
    report = {"records": int(back[0]), "end_offset": int(back[1]), "segments": int(back[2]), "wrong_guesses": int(back[3]),
              "repair_rounds": int(back[4]), "error": int(back[5]), "error_offset": int(back[6])}
    if entries is not None:
        report["segment_entries"] = entries
    return offsets[: report["records"]], report


# the arrays `rocco_hip_bam_record_fields` writes, in its order, with the names of their torch dtypes
_FIELD_DTYPES = tuple((name, _rt._tensor_dtype(name, dtype)) for name, dtype in (("tid", np.int32),) + _rt._RECORD_FIELDS + (_rt._QLEN_FIELD,))


def record_fields_device(bytes_t, offsets_t, n_ref: int):
    """`rocco_hip_bam_record_fields`: ({field: CUDA tensor} for tid, pos, end, isize, flag (the uint16 bit pattern as int16),
    mapq, mate_same, qlen; the n_ref + 2 contig offsets; (error code, record index))."""
    import torch

    lib = _native.load()
    bytes_t, offsets_t = bytes_t.contiguous(), offsets_t.contiguous()
    n = int(offsets_t.shape[0])
    out = {name: torch.empty(n, dtype=getattr(torch, dtype), device=bytes_t.device) for name, dtype in _FIELD_DTYPES}
    firsts, back = (ctypes.c_longlong * (int(n_ref) + 2))(), (ctypes.c_longlong * 2)()
    _native.check(lib.rocco_hip_bam_record_fields(
        _native.solver_for(bytes_t.device.index).handle, bytes_t.data_ptr(), int(bytes_t.shape[0]), offsets_t.data_ptr(), n, int(n_ref),
        *[out[name].data_ptr() for name, _ in _FIELD_DTYPES], firsts, back, _dp._stream_ptr(bytes_t)), "rocco_hip_bam_record_fields")
    return out, [int(v) for v in firsts], (int(back[0]), int(back[1]))


def _record_error(name: str, code: int, record: int, offset: int) -> ValueError:
    return ValueError(f"{name}: record {record} at byte {offset} of the inflated stream: {_ERROR_TEXT.get(code, f'error {code}')}")


def decode_records_device(bytes_t, entry0: int, n_ref: int, segment_bytes: Optional[int] = None, guess_mode: int = 1, name: str = "<bytes>",
                          whole: bool = True, first_record: int = 0, first_byte: int = 0):
    """Walk plus fields over one inflated stream (or slab) on the device, every error code turned into a ValueError that
    names ``name``, the record index and the byte offset.  ``whole``: the stream must end behind a complete record (else
    the bytes behind ``report["end_offset"]`` belong in front of the next slab).  Returns (fields, contig offsets, report)."""
    offsets, report = walk_records_device(bytes_t, entry0, n_ref, segment_bytes, guess_mode)
    if report["error"] == ERR_BLOCK_SIZE or (report["error"] == ERR_TRUNCATED and whole):
        raise _record_error(name, report["error"], first_record + report["records"], first_byte + report["error_offset"])
    fields, firsts, (code, record) = record_fields_device(bytes_t, offsets, n_ref)
    if code:
        raise _record_error(name, code, first_record + record, first_byte + int(offsets[record]))
    return fields, firsts, report


def stream_firsts_device(offsets_t, tid_t, bounds, expect_tid):
    """`rocco_hip_bam_stream_firsts`: splits the walked chain of K streams laid one behind the other back into its streams.
    ``offsets_t`` / ``tid_t``: the int64 record offsets and int32 reference ids as CUDA tensors; ``bounds``: the K + 1 ascending
    byte bounds; ``expect_tid``: the K reference ids.  Returns (the K + 1 first records as a list, (error code, stream))."""
    import torch

    lib = _native.load()
    if not _dp._is_tensor(offsets_t) or offsets_t.dtype != torch.int64 or not offsets_t.is_cuda or not _dp._is_tensor(tid_t) or \
            tid_t.dtype != torch.int32 or tid_t.device != offsets_t.device or tid_t.shape != offsets_t.shape or offsets_t.dim() != 1:
        raise TypeError("stream_firsts_device: an int64 and an int32 CUDA tensor of one length on one device are required")
    offsets_t, tid_t = offsets_t.contiguous(), tid_t.contiguous()
    K, n = len(expect_tid), int(offsets_t.shape[0])
    if K < 1 or len(bounds) != K + 1:
        raise ValueError("stream_firsts_device: K >= 1 expected reference ids and K + 1 bounds are required")
    bounds_c, expect_c = (ctypes.c_longlong * (K + 1))(*[int(b) for b in bounds]), (ctypes.c_int * K)(*[int(t) for t in expect_tid])
    firsts, back = (ctypes.c_longlong * (K + 1))(), (ctypes.c_longlong * 2)()
    with torch.cuda.device(offsets_t.device):
        _native.check(lib.rocco_hip_bam_stream_firsts(
            _native.solver_for(offsets_t.device.index).handle, offsets_t.data_ptr() if n else None, tid_t.data_ptr() if n else None, n,
            bounds_c, expect_c, K, firsts, back, _dp._stream_ptr(offsets_t)), "rocco_hip_bam_stream_firsts")
    return [int(v) for v in firsts], (int(back[0]), int(back[1]))


def _decode_slabs(slabs, entry0: int, n_ref: int, segment_bytes: Optional[int], guess_mode: int, name: str, dev, cut_tail: int = 0):
    """The slab loop of `read_alignment_file` and of a span too large for one group (`read_alignment_spans`): walks and decodes
    ``slabs`` (device tensors of inflated bytes, at least one) from ``entry0`` of the first; a slab's bytes behind its last
    complete record are carried, on the device, in front of the next; the last slab loses its last ``cut_tail`` bytes and must
    end behind a complete record.  Returns (the fields of every slab, the records per contig -- those without one last --,
    the walk's totals)."""
    import torch

    carry = empty = torch.empty(0, dtype=torch.uint8, device=dev)  # (what the walk has not consumed yet, in front of the next slab)
    parts, counts, last_key, n_records, consumed = [], np.zeros(n_ref + 1, dtype=np.int64), -1, 0, 0
    totals = {"records": 0, "segments": 0, "wrong_guesses": 0, "repair_rounds": 0, "slabs": 0}

    def with_last(it):  # (the header needs a block, so there is a slab)
        previous = next(it)
        for item in it:
            yield previous, False
            previous = item
        yield previous, True

    for slab, is_last in with_last(iter(slabs)):
        if is_last and cut_tail:
            slab = slab[: slab.shape[0] - cut_tail]
        data = torch.cat([carry, slab]) if carry.shape[0] else slab
        if data.shape[0] < entry0 and not is_last:  # (the header straddles slabs)
            carry = data
            continue
        fields, firsts, rep = decode_records_device(data, entry0, n_ref, segment_bytes, guess_mode, name, whole=is_last,
                                                    first_record=n_records, first_byte=consumed)
        slab_counts = np.diff(np.asarray(firsts, dtype=np.int64))
        present = np.flatnonzero(slab_counts)
        if present.size:
            if int(present[0]) < last_key:
                raise _record_error(name, ERR_ORDER, n_records, consumed + entry0)
            last_key = int(present[-1])
        counts += slab_counts
        parts.append(fields)
        n_records += rep["records"]
        for key in ("records", "segments", "wrong_guesses", "repair_rounds"):
            totals[key] += rep[key]
        totals["slabs"] += 1
        carry = data[rep["end_offset"]:].clone() if rep["end_offset"] < data.shape[0] else empty
        consumed += rep["end_offset"]
        entry0 = 0
    return parts, counts, totals


def read_alignment_file(path, device=None, names=None, slab_bytes: int = DEFAULT_SLAB_BYTES, segment_bytes: Optional[int] = None,
                        threads: Optional[int] = None, guess_mode: int = 1, report: Optional[dict] = None, inflate: str = "host"):
    """A whole BAM file as (`AlignmentFileRecords` whose records carry ``qlen`` and are CUDA tensors, ``name`` the path; the
    number of records without a contig).  The file is read and its block headers are walked once; the header comes first, from
    a host inflate of the leading blocks it covers (so a file with a bad header reports the header, whatever else is wrong
    with it).  Then slab by slab: about ``slab_bytes`` inflated bytes arrive as a uint8 tensor on the device -- inflated on the
    host and uploaded (``inflate="host"``, on ``threads`` threads) or inflated where they are consumed (``inflate="device"``:
    the inflated bytes never visit the host) -- and are walked and decoded there; a slab's bytes behind its last complete
    record are carried, on the device, in front of the next slab; the per-contig arrays are views of the seven concatenated
    arrays.  ``names``: keep these contigs only.  ``report`` (a dict) receives the walk's totals.  The decoded arrays are the
    same in both modes."""
    import torch

    path = os.fspath(path)
    if inflate not in ("host", "device"):
        raise ValueError(f"read_alignment_file: inflate must be \"host\" or \"device\", not {inflate!r}")
    dev = _dp._device(device)
    raw, _, blocks, slab_bytes = _bgzf_front(path, max(1, int(slab_bytes)), "read_alignment_file")
    contigs, entry0 = _header_from_leading_blocks(raw, path, blocks)
    if inflate == "device":
        slabs = _inflate_slabs_device(raw, path, blocks, dev, slab_bytes)
    else:
        slabs = _uploaded(_inflate_slabs(raw, path, blocks, threads, slab_bytes), dev)
    n_ref = len(contigs)
    parts, counts, totals = _decode_slabs(slabs, entry0, n_ref, segment_bytes, guess_mode, path, dev)
    if report is not None:
        report.update(totals)
    whole = {name: (torch.cat([p[name] for p in parts]) if len(parts) > 1 else parts[0][name]) for name, _ in _FIELD_DTYPES}
    firsts = np.concatenate([[0], np.cumsum(counts)])
    keep = None if names is None else {str(n) for n in names}
    records = {}
    for k, (contig, _) in enumerate(contigs):
        if keep is not None and contig not in keep:
            continue
        lo, hi = int(firsts[k]), int(firsts[k + 1])
        # (the kernel checked every value: no second pass over the arrays)
        records[contig] = AlignmentRecords._of(*[whole[field][lo:hi] for field in AlignmentRecords.__slots__])
    return AlignmentFileRecords(contigs, records, name=path), int(counts[n_ref])


# --------------------------------------------------------------------------------------------
# contigs of files read through the .bai index: K streams, one device pass (note (32))
# --------------------------------------------------------------------------------------------

class _LeadingBlocks:
    """The block rows of a file from its first, walked as `_header_from_leading_blocks` asks for them (the words of
    `_bgzf_blocks`): the header of an indexed file costs its leading blocks, not a walk over every block header."""

    def __init__(self, raw, name: str):
        self.raw, self.name, self.rows, self.at, self.asked = raw, name, [], 0, 0

    def _grow(self, k: int) -> None:
        def bad(what: str) -> ValueError:
            return ValueError(f"{_block_where(self.name, len(self.rows), self.at)}: {what}")

        while len(self.rows) <= k and self.at < len(self.raw):
            self.rows.append(_bgzf_block_at(self.raw, len(self.raw), self.at, bad))
            self.at = self.rows[-1][2] + 8

    def __len__(self) -> int:
        self._grow(self.asked)
        return len(self.rows)

    def __getitem__(self, k: int):
        self.asked = max(self.asked, k + 1)
        self._grow(k)
        return self.rows[k]


def _mapped_bytes(path: str):
    """The file's bytes, mapped: a span's blocks are read where they are used, the rest of the file is not."""
    if os.path.getsize(path) == 0:
        return memoryview(b"")
    return memoryview(np.memmap(path, dtype=np.uint8, mode="r"))


class _BamFront:
    """What is kept of an indexed file between calls: its header's ``contigs``, ``tid_of`` (name -> reference id) and its
    parsed ``index``."""

    def __init__(self, path: str, contigs, index):
        self.path, self.contigs, self.index = path, contigs, index
        self.tid_of = {name: tid for tid, (name, _) in reversed(list(enumerate(contigs)))}


_BAM_FRONT_CACHE: "collections.OrderedDict" = collections.OrderedDict()
BAM_FRONT_CACHE_FILES = 1024


def _file_key(path: str):
    stat = os.stat(path)
    return (os.path.abspath(path), int(stat.st_size), int(stat.st_mtime_ns))


def _bam_front(path: str) -> Optional[_BamFront]:
    """The header and the index of ``path`` (cached on the file's and the index's (path, size, mtime)); None without an index."""
    index = _bai.open_bam_index(path)
    if index is None:
        return None
    key = _file_key(path) + (index.name, index.size, id(index))
    hit = _BAM_FRONT_CACHE.get(key)
    if hit is not None:
        _BAM_FRONT_CACHE.move_to_end(key)
        return hit
    raw = _mapped_bytes(path)
    contigs, _ = _header_from_leading_blocks(raw, path, _LeadingBlocks(raw, path))
    front = _BAM_FRONT_CACHE[key] = _BamFront(path, contigs, index)
    while len(_BAM_FRONT_CACHE) > BAM_FRONT_CACHE_FILES:
        _BAM_FRONT_CACHE.popitem(last=False)
    return front


class _Stream:
    """One (file, contig) of `read_alignment_spans`: its blocks, the bytes to skip in the first and to keep of the last."""

    __slots__ = ("path", "contig", "tid", "n_ref", "raw", "blocks", "skip", "keep", "size", "index_name")

    def where(self) -> str:
        return f"{self.path}: contig {self.contig}"


def _not_this_file(stream: "_Stream", found: str) -> ValueError:
    return ValueError(f"{stream.where()}: {found}; the index {stream.index_name} does not describe this file")


def _span_streams(wanted) -> List["_Stream"]:
    raws, out = {}, []
    for path, contig in wanted:
        path, contig = os.fspath(path), str(contig)
        front = _bam_front(path)
        if front is None:
            raise ValueError(f"{path}: read_alignment_spans needs its .bai index (read_alignment_file reads a file without one)")
        if contig not in front.tid_of:
            raise KeyError(f"{path}: no contig {contig}")
        s = _Stream()
        s.path, s.contig, s.tid, s.n_ref, s.index_name = path, contig, front.tid_of[contig], len(front.contigs), front.index.name
        span = _bai.contig_span(front.index, s.tid)
        s.raw, s.blocks, s.skip, s.keep, s.size = None, [], 0, 0, 0
        if span is not None:
            if path not in raws:
                raws[path] = _mapped_bytes(path)
            s.raw = raws[path]
            s.blocks, s.skip, s.keep = _bgzf_span_blocks(s.raw, path, contig, span[0], span[1])
            if s.blocks:
                s.size = sum(b[4] for b in s.blocks) - s.skip - (s.blocks[-1][4] - s.keep)
                if s.size < 0:
                    raise _not_this_file(s, f"its span ends at virtual offset {span[1]}, before its begin {span[0]}")
        out.append(s)
    return out


def _span_groups(streams, batch_bytes: int):
    """(first, one past the last) stream of every group: a group's inflated bytes stay under ``batch_bytes`` (a stream that
    alone exceeds it is a group of its own and goes through the slab loop); its streams share one header length (the record
    checks take ``n_ref``) and their reference ids do not descend (the record checks demand the order of a sorted file)."""
    first = 0
    while first < len(streams):
        last, size, tid = first + 1, streams[first].size, (streams[first].tid if streams[first].size else -1)
        while last < len(streams) and streams[first].size <= batch_bytes:
            nxt = streams[last]
            if nxt.n_ref != streams[first].n_ref or size + nxt.size > batch_bytes or (nxt.size and nxt.tid < tid):
                break
            size, tid, last = size + nxt.size, (nxt.tid if nxt.size else tid), last + 1
        yield first, last
        first = last


def _group_layout(group):
    """ONE block table and one compressed buffer for the blocks of the group's streams: (the table, the span list, per row its
    (stream, block index, file offset), per stream the slice of the inflated bytes that is its own); a block that two
    neighbouring streams share has one row."""
    rows, owner, spans, out_at = [], [], SpanList(), 0
    slices = []
    for k, s in enumerate(group):
        if not s.blocks:
            slices.append((0, 0))
            continue
        refuse_large_blocks(s.blocks, lambda index, block: _block_where(s.path, index, block[0]))
        first_row = None
        for index, block in enumerate(s.blocks):
            if index == 0 and owner and owner[-1][0].raw is s.raw and owner[-1][2] == block[0]:
                first_row = len(rows) - 1  # (the block the stream before ends in)
                continue
            lo, hi = block[1], block[2]
            comp_at = spans.add(s.raw, lo, hi, max_gap=64)  # (neighbours: the trailer and the next header ride along)
            if first_row is None:
                first_row = len(rows)
            rows.append((comp_at, comp_at + hi - lo, block[4], block[3], out_at))
            owner.append((s, index, block[0]))
            out_at += block[4]
        last_row = len(rows) - 1
        slices.append((rows[first_row][4] + s.skip, rows[last_row][4] + s.keep))
    return np.asarray(rows, dtype=np.int64).reshape(-1, BGZF_TABLE_COLUMNS), spans, owner, slices


def _group_bytes_device(group, dev):
    """The useful bytes of the group's streams, one behind the other, from the one table of `_group_layout`, one pinned
    staging buffer, one upload and one `rocco_hip_bgzf_inflate`."""
    import torch

    table, spans, owner, slices = _group_layout(group)
    with torch.cuda.device(dev):
        table_t, comp_t = upload_blocks(table, spans.spans, spans.n_comp, dev)
        out = torch.empty(int(table[:, 2].sum()), dtype=torch.uint8, device=dev)
        _, report = inflate_blocks_device(comp_t, table_t, out)  # (synchronises: the upload's pinned buffer may go)
        if report["block"] >= 0:
            s, index, offset = owner[report["block"]]
            raise _bgzf_error(f"{_block_where(s.path, index, offset)} (blocks counted from the span of contig {s.contig})",
                              int(table[report["block"], 2]), report)
        pieces = [out[lo:hi] for lo, hi in slices if hi > lo]
        if len(pieces) == 1:
            return pieces[0]
        return torch.cat(pieces) if pieces else out[:0]


def _group_bytes_host(group, dev, threads: Optional[int]):
    """The same bytes from a host inflate: every block's useful bytes are placed directly at their final place in one pinned
    buffer, which goes up in one copy."""
    import torch

    jobs, at = [], 0
    for s in group:
        for index, block in enumerate(s.blocks):
            lo = s.skip if index == 0 else 0
            hi = s.keep if index == len(s.blocks) - 1 else block[4]
            jobs.append((s, index, block, lo, hi, at))
            at += max(hi - lo, 0)
    out = _host_buffer(at)

    def one(job):
        s, index, block, lo, hi, to = job
        data = _inflate_block(s.raw, s.path, index, block)
        if hi > lo:
            out[to: to + hi - lo] = np.frombuffer(data, dtype=np.uint8)[lo:hi]

    on_pool(one, jobs, threads)
    with torch.cuda.device(dev):
        (up,) = _uploaded([out], dev)  # (waits for the copy: the pinned `out` may go)
    return up


def _decode_group(group, dev, inflate: str, segment_bytes: Optional[int], threads: Optional[int]):
    """One inflate, one walk, one field decode and one split for the streams of a group: ({field: tensor}, the K + 1 first
    records)."""
    data = _group_bytes_device(group, dev) if inflate == "device" else _group_bytes_host(group, dev, threads)
    bounds = [0]
    for s in group:
        bounds.append(bounds[-1] + s.size)
    if int(data.shape[0]) != bounds[-1]:
        raise RuntimeError(f"read_alignment_spans: {int(data.shape[0])} bytes laid out where the spans hold {bounds[-1]}")

    def stream_at(offset: int) -> int:
        return min(max(bisect.bisect_right(bounds, offset) - 1, 0), len(group) - 1)

    n_ref = group[0].n_ref
    offsets, report = walk_records_device(data, 0, n_ref, segment_bytes)
    if report["error"]:
        k = stream_at(report["error_offset"])
        raise _not_this_file(group[k], f"the record at byte {report['error_offset'] - bounds[k]} of its span, as the index states it: "
                             f"{_ERROR_TEXT[report['error']]} (or the file is damaged there)")
    fields, _, (code, record) = record_fields_device(data, offsets, n_ref)
    firsts, (split_code, stream) = stream_firsts_device(offsets, fields["tid"], bounds, [s.tid for s in group])
    if split_code == ERR_SEAM:
        raise _not_this_file(group[stream], "no record begins where its span begins, or the span before it ends inside a record")
    if split_code:
        k, lo, hi = stream, firsts[stream], firsts[stream + 1]
        other = fields["tid"][lo:hi]
        other = other[other != group[k].tid]
        found = int(other[0]) if other.numel() else -1
        raise _not_this_file(group[k], f"a record of its span lies on reference {found}, the contig is reference {group[k].tid}")
    if code:
        at = int(offsets[record])
        k = stream_at(at)
        raise ValueError(f"{group[k].where()}: record {record - firsts[k]} of the contig, at byte {at - bounds[k]} of its span: "
                         f"{_ERROR_TEXT.get(code, f'error {code}')}")
    return fields, firsts


def _decode_long_stream(s: "_Stream", dev, inflate: str, segment_bytes: Optional[int], threads: Optional[int], slab_bytes: int):
    """A stream that alone exceeds a group's budget: the slab loop of `read_alignment_file` from the span's entry, cut at its end."""
    slab_bytes = max(1, int(slab_bytes))
    if inflate == "device":
        slabs = _inflate_slabs_device(s.raw, s.path, s.blocks, dev, slab_bytes)
    else:
        slabs = _uploaded(_inflate_slabs(s.raw, s.path, s.blocks, threads, slab_bytes), dev)
    try:
        parts, counts, _ = _decode_slabs(slabs, s.skip, s.n_ref, segment_bytes, 1, s.path, dev, cut_tail=s.blocks[-1][4] - s.keep)
    except ValueError as exc:
        raise _not_this_file(s, f"its span does not decode ({exc})") from None
    elsewhere = [k for k in np.flatnonzero(counts).tolist() if k != s.tid]
    if elsewhere:
        found = elsewhere[0] if elsewhere[0] < s.n_ref else -1
        raise _not_this_file(s, f"a record of its span lies on reference {found}, the contig is reference {s.tid}")
    return parts


def read_alignment_spans(wanted, device=None, inflate: Optional[str] = None, segment_bytes: Optional[int] = None,
                         batch_bytes: int = DEFAULT_BATCH_BYTES, threads: Optional[int] = None) -> List[AlignmentRecords]:
    """The records of every ``(path, contig)`` of ``wanted`` -- several contigs of one file, one contig of K files, any mix --
    through the files' ``.bai`` indexes: one `AlignmentRecords` with ``qlen`` per pair, as CUDA tensors, views of seven
    concatenated arrays, the same values `read_alignment_file` gives for the contig.  Only the BGZF blocks between the virtual
    offsets the index names for a contig are read (`rocco_amd.bam_index.contig_span`); a contig without a span gives empty
    records; KeyError for a contig the file's header does not name, ValueError for a file without a ``.bai``.

    The streams are grouped (`_span_groups`: under ``batch_bytes`` inflated bytes, `DEFAULT_BATCH_BYTES`); every group costs
    one inflate (``inflate="device"``: one block table, one upload, one `rocco_hip_bgzf_inflate`; ``"host"``: the thread pool
    places every block's useful bytes in one pinned buffer, one upload; default `DEFAULT_INFLATE`), one
    `rocco_hip_bam_walk_records` over the useful bytes of its streams laid one behind the other -- each begins and ends on a
    record boundary, so they form one record chain --, one `rocco_hip_bam_record_fields` and one
    `rocco_hip_bam_stream_firsts`, which splits the chain back and checks what the index claimed: every stream begins on a
    record start and holds records of its contig only.  A stream that alone exceeds ``batch_bytes`` goes through the slab loop
    of `read_alignment_file`.  An index that does not describe its file (an offset inside a record, spans of other contigs,
    another file's index) is a ValueError naming the file and the contig."""
    import torch

    inflate = DEFAULT_INFLATE if inflate is None else inflate
    if inflate not in ("host", "device"):
        raise ValueError(f"read_alignment_spans: inflate must be \"host\" or \"device\", not {inflate!r}")
    batch_bytes = int(batch_bytes)
    if batch_bytes < 1:
        raise ValueError("read_alignment_spans: batch_bytes must be positive")
    dev = _dp._device(device)
    streams = _span_streams(list(wanted))
    parts, lengths = [], []  # the fields of every group (or slab), and per stream its record count
    with torch.cuda.device(dev):
        for first, last in _span_groups(streams, batch_bytes):
            group = streams[first:last]
            if not any(s.size for s in group):
                lengths += [0] * len(group)
            elif len(group) == 1 and group[0].size > batch_bytes:
                slabs = _decode_long_stream(group[0], dev, inflate, segment_bytes, threads, batch_bytes)
                parts += slabs
                lengths.append(sum(int(p["pos"].shape[0]) for p in slabs))
            else:
                fields, firsts = _decode_group(group, dev, inflate, segment_bytes, threads)
                parts.append(fields)
                lengths += np.diff(firsts).tolist()
        names = [name for name in AlignmentRecords.__slots__]
        if parts:
            whole = {name: (torch.cat([p[name] for p in parts]) if len(parts) > 1 else parts[0][name]) for name in names}
        else:
            whole = {name: torch.empty(0, dtype=getattr(torch, dtype), device=dev) for name, dtype in _FIELD_DTYPES if name in names}
    out, at = [], 0
    for n in lengths:
        out.append(AlignmentRecords._of(*[whole[name][at: at + n] for name in names]))
        at += n
    return out


# --------------------------------------------------------------------------------------------
# decoded files kept on the device (generate_chrom_matrix asks once per file and chromosome)
# --------------------------------------------------------------------------------------------

ALIGNMENT_CACHE_BYTES = 8 << 30  # the budget: 20 bytes per record; least recently used files (or contigs of indexed files) leave first
_ALIGNMENT_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_INDEXED_FILES: dict = {}  # the `IndexedAlignmentFile` of a file key: a header and an index, no records
_BAM_COUNT_METADATA_CACHE: dict = {}


def clear_alignment_cache() -> None:
    """Drops every decoded file, every decoded contig of an indexed file (and the metadata derived from them)."""
    _ALIGNMENT_CACHE.clear()
    _INDEXED_FILES.clear()
    _BAM_COUNT_METADATA_CACHE.clear()


def _file_bytes(file: AlignmentFileRecords) -> int:
    return 20 * sum(len(r) for r in file.records.values())


def _evict() -> None:
    while len(_ALIGNMENT_CACHE) > 1 and sum(s for _, s in _ALIGNMENT_CACHE.values()) > ALIGNMENT_CACHE_BYTES:
        _ALIGNMENT_CACHE.popitem(last=False)


class _ContigRecords(collections.abc.Mapping):
    """``IndexedAlignmentFile.records``: a mapping over the header's names; a contig is decoded when it is asked for."""

    def __init__(self, file: "IndexedAlignmentFile"):
        self._file = file

    def __contains__(self, contig) -> bool:  # (membership is the header's: nothing is decoded)
        return contig in self._file.tid_of

    def __iter__(self):
        return iter(name for name, _ in self._file.contigs)

    def __len__(self) -> int:
        return len(self._file.contigs)

    def __getitem__(self, contig) -> AlignmentRecords:
        if contig not in self._file.tid_of:
            raise KeyError(contig)
        return self._file.load([contig])[0]


class _LazyTracks:
    """``IndexedAlignmentFile.tracks()``: (contig, records) in header order, contigs without records left out, each decoded
    when the iteration reaches it -- a probe that stops early (`rocco_amd.readtracks._head_chunks`) decodes the leading
    contigs it reaches and no more."""

    carries_qlen = True  # (records read through the index always carry `qlen`)

    def __init__(self, file: "IndexedAlignmentFile"):
        self._file = file

    def __iter__(self):
        for name, _ in self._file.contigs:
            if self._file.count(name) == 0:
                continue
            records = self._file.records[name]
            if len(records) > 0:
                yield name, records


class IndexedAlignmentFile(AlignmentFileRecords):
    """A BAM file with a ``.bai`` index as `AlignmentFileRecords`: the header's ``contigs`` and the ``index``
    (`rocco_amd.bam_index.BamIndex`), no records until they are asked for.  ``records`` is a mapping over the header's names
    (membership is the header's, as for a decoded file); a contig is decoded on first access through `read_alignment_spans`
    and kept in the alignment cache per contig.  `count` answers the length of a contig from the index statistics without
    decoding; `load` fetches several contigs in one call; `tracks()` is lazy."""

    def __init__(self, path: str, front: "_BamFront", key):
        AlignmentFileRecords.__init__(self, front.contigs, {}, name=path)
        self.path, self.index, self.tid_of, self.key = path, front.index, front.tid_of, key
        self.records = _ContigRecords(self)

    def count(self, contig: str) -> Optional[int]:
        """The records of the contig by the index statistics (mapped + unmapped); 0 for a contig without a span; None where
        the index has a span and no statistics for it."""
        tid = self.tid_of[contig]
        if _bai.contig_span(self.index, tid) is None:
            return 0
        stats = _bai.contig_stats(self.index, tid)
        return None if stats is None else int(stats[0] + stats[1])

    def index_read_counts(self, exclude_chromosomes=()) -> Optional[Tuple[int, int]]:
        """(mapped, unmapped) summed over the contigs not in ``exclude_chromosomes`` from the index statistics, as the
        reference's ``ccounts_getMappedReadCount`` takes them (``hts_idx_get_stat``); None for an index without pseudo-bins."""
        excluded, mapped, unmapped = {str(c) for c in (exclude_chromosomes or ())}, 0, 0
        for name, _ in self.contigs:
            if name in excluded or _bai.contig_span(self.index, self.tid_of[name]) is None:
                continue
            stats = _bai.contig_stats(self.index, self.tid_of[name])
            if stats is None:
                return None
            mapped, unmapped = mapped + int(stats[0]), unmapped + int(stats[1])
        return mapped, unmapped

    def load(self, names) -> List[AlignmentRecords]:
        """The records of ``names``: those not in the cache are read in ONE `read_alignment_spans` call."""
        return _load_contigs([(self, str(n)) for n in names])

    def tracks(self, names=None):
        """(contig, records), contigs without records left out: lazily in header order, or for ``names`` in their order,
        fetched in one call."""
        if names is None:
            return _LazyTracks(self)
        names = [n for n in names if n in self.tid_of]
        return [(n, r) for n, r in zip(names, self.load(names)) if len(r) > 0]


def _load_contigs(pairs) -> List[AlignmentRecords]:
    """The records of every (`IndexedAlignmentFile`, contig): from the per-contig cache, the rest from ONE
    `read_alignment_spans` call, kept under `ALIGNMENT_CACHE_BYTES` (least recently used entries leave first)."""
    out, missing = [None] * len(pairs), []
    for i, (file, contig) in enumerate(pairs):
        hit = _ALIGNMENT_CACHE.get(file.key + (contig,))
        if hit is not None:
            _ALIGNMENT_CACHE.move_to_end(file.key + (contig,))
            out[i] = hit[0]
        else:
            missing.append(i)
    if missing:
        order = {}
        for i in missing:  # (a pair asked for twice is read once)
            order.setdefault((pairs[i][0].key, pairs[i][1]), i)
        first = list(order.values())
        read = read_alignment_spans([(pairs[i][0].path, pairs[i][1]) for i in first], inflate=DEFAULT_INFLATE)
        by_key = {}
        for i, records in zip(first, read):
            by_key[(pairs[i][0].key, pairs[i][1])] = records
            _ALIGNMENT_CACHE[pairs[i][0].key + (pairs[i][1],)] = (records, 20 * len(records))
        for i in missing:
            out[i] = by_key[(pairs[i][0].key, pairs[i][1])]
        _evict()
    return out


def _cached_file(bam_file: str) -> AlignmentFileRecords:
    key = _file_key(bam_file)
    if USE_INDEX:
        front = _bam_front(bam_file)
        if front is not None:
            key = key + (front.index.name, front.index.size)
            file = _INDEXED_FILES.get(key)
            if file is None or file.index is not front.index:
                file = _INDEXED_FILES[key] = IndexedAlignmentFile(bam_file, front, key)
            return file
    hit = _ALIGNMENT_CACHE.get(key)
    if hit is not None:
        _ALIGNMENT_CACHE.move_to_end(key)
        return hit[0]
    file, _ = read_alignment_file(bam_file, inflate=DEFAULT_INFLATE)
    file.name = bam_file
    size = _file_bytes(file)
    _ALIGNMENT_CACHE[key] = (file, size)
    _evict()
    return file


def _resolve_num_processors(num_processors) -> int:
    """rocco/readtracks.py:45-48 (the ``threads`` key of the metadata and of its cache key; nothing here runs on them)."""
    if num_processors is None or int(num_processors) < 1:
        return max(multiprocessing.cpu_count() - 1, 1)
    return int(num_processors)


def _clean_string(text) -> str:
    return "" if text is None else text.lower().replace(" ", "")


def _get_bam_count_metadata(bam_file: str, step: int, norm_method: str, effective_genome_size: float, ignore_for_norm,
                            flag_exclude: int = 0, extend_reads: int = -1, num_processors: int = 1, scale_factor: float = 1.0) -> dict:
    """rocco/readtracks.py:242-353 with the same signature, dict, log lines and cache key, from the file's decoded records
    (`bam_count_metadata_from_records`)."""
    ignore = tuple(ignore_for_norm or [])
    threads = _resolve_num_processors(num_processors)
    cache_key = (bam_file, int(step), _clean_string(norm_method).upper(), float(effective_genome_size if effective_genome_size is not None else -1.0),
                 ignore, int(flag_exclude), int(extend_reads), int(threads), float(scale_factor))
    if cache_key in _BAM_COUNT_METADATA_CACHE:
        return _BAM_COUNT_METADATA_CACHE[cache_key]
    metadata = dict(_rt.bam_count_metadata_from_records(_cached_file(bam_file), step, norm_method, effective_genome_size, list(ignore),
                                                        flag_exclude=flag_exclude, extend_reads=extend_reads, scale_factor=scale_factor,
                                                        bam_file=bam_file))
    metadata["threads"] = int(threads)
    _BAM_COUNT_METADATA_CACHE[cache_key] = metadata
    return metadata


def get_bam_chrom_reads(bam_file: str, chromosome: str, chrom_sizes_file: str, step: int, effective_genome_size: float = -1,
                        norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                        extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                        num_processors: int = -1, const_scale: float = 1.0, round_digits: int = 5, scale_by_step: bool = False):
    """rocco/readtracks.py:389-518 with the same signature, return value, errors and warnings: the file is decoded once
    (`read_alignment_file`, kept on the device), the rest is `bam_chrom_reads_from_records`."""
    if not os.path.exists(bam_file):
        raise FileNotFoundError(f"BAM file not found: {bam_file}")
    if not os.path.exists(chrom_sizes_file):
        raise FileNotFoundError(f"Chromosome sizes file not found: {chrom_sizes_file}")
    sizes = _rt.get_chroms_and_sizes(chrom_sizes_file)
    if chromosome not in sizes:
        raise ValueError(f"Chromosome {chromosome} not found in chromosome sizes file: {chrom_sizes_file}")
    if ignore_for_norm is None:
        ignore_for_norm = ["chrX", "chrY", "chrM"]
    metadata = _get_bam_count_metadata(bam_file, step=step, norm_method=norm_method, effective_genome_size=effective_genome_size,
                                       ignore_for_norm=ignore_for_norm, flag_exclude=flag_exclude, extend_reads=extend_reads,
                                       num_processors=num_processors, scale_factor=scale_factor)
    file = _cached_file(bam_file)
    if chromosome not in file.records:
        logger.warning("Chromosome %s not found in BAM file: %s. Returning (None,None).", chromosome, bam_file)
        return None, None
    return _rt.bam_chrom_reads_from_records(file.records[chromosome], int(sizes[chromosome]), step, metadata,
                                            min_mapping_score=min_mapping_score, flag_include=flag_include, flag_exclude=flag_exclude,
                                            center_reads=center_reads, const_scale=const_scale, round_digits=round_digits,
                                            scale_by_step=scale_by_step, bam_file=bam_file, chromosome=chromosome)


# --------------------------------------------------------------------------------------------
# K files of one chromosome -> its count matrix in one device pass
# --------------------------------------------------------------------------------------------

class _HeldRecords(logging.Filter):
    """Keeps the records the module's logger would emit, for `logger.handle` to emit later in the reference's order."""

    def __init__(self):
        super().__init__()
        self.records = []

    def filter(self, record):
        self.records.append(record)
        return False


def _prefetch_chromosome(input_files, chromosome: str, chrom_sizes_file: str) -> None:
    """The chromosome's records of every indexed file among ``input_files`` into the cache, in ONE `read_alignment_spans` call
    (files without an index keep the whole-file route).  Nothing is fetched where a file or the chromosome is missing, and an
    error raised here is dropped: it belongs to its file's own turn in the loop that follows, in the reference's order."""
    if not USE_INDEX or not os.path.exists(chrom_sizes_file) or not all(os.path.exists(f) for f in input_files):
        return
    try:
        if chromosome not in _rt.get_chroms_and_sizes(chrom_sizes_file):
            return
        pairs = []
        for bam_file in input_files:
            if _bai.bam_index_path(bam_file) is not None:
                file = _cached_file(bam_file)
                if isinstance(file, IndexedAlignmentFile) and chromosome in file.records:
                    pairs.append((file, chromosome))
        if pairs:
            _load_contigs(pairs)
    except (ValueError, KeyError, OSError):
        return


def generate_chrom_matrix_device(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, const_scale: float = 1.0,
                                 round_digits: int = 5, scale_by_step: bool = False, effective_genome_size: float = -1,
                                 norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                                 extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                                 num_processors: int = -1, low_memory: bool = False):
    """The reference's ``generate_chrom_matrix`` over BAM files (rocco/readtracks.py:521-633, same keywords) with the matrix
    left on the device: returns (starts as a host ``int`` array, count matrix as a CUDA tensor), or ``(None, None)``.  Per
    file, in file order, what ``get_bam_chrom_reads`` does before it counts -- its two FileNotFoundErrors and its
    chromosome ValueError for the first offending file, the metadata through `_get_bam_count_metadata` (its cache, its log
    lines), the decoded file from `_cached_file`, the warning for a header without the contig --; everything after that
    for all files at once (`rocco_amd.readtracks.bam_chrom_matrix_from_records_batch`: two waits for the device per call,
    nothing as long as the chromosome on the bus).  The log records of the call are the reference's, in its order: they are
    held while the files are worked on together and emitted file by file afterwards.  This is the function to bind behind
    ``rocco_amd.rocco.generate_chrom_matrix``."""
    track_types = {_rt._get_track_type(input_file) for input_file in input_files}
    if len(track_types) != 1:
        raise ValueError("All input files must share the same type.")
    if next(iter(track_types)) != "bam":
        raise ValueError("rocco_amd.bam.generate_chrom_matrix reads BAM files: bigWig inputs go through "
                         "rocco_amd.readtracks.generate_chrom_matrix")
    threads = max((os.cpu_count() or 2) - 1, 1) if (num_processors is None or int(num_processors) < 1) else int(num_processors)
    if ignore_for_norm is None:
        ignore_for_norm = ["chrX", "chrY", "chrM"]
    K = len(input_files)
    _prefetch_chromosome(input_files, chromosome, chrom_sizes_file)
    before, records_list, metadata_list, present, chrom_size = [[] for _ in range(K)], [], [], [], 0
    held = _HeldRecords()
    logger.addFilter(held)
    try:
        for k, bam_file in enumerate(input_files):
            if not os.path.exists(bam_file):
                raise FileNotFoundError(f"BAM file not found: {bam_file}")
            if not os.path.exists(chrom_sizes_file):
                raise FileNotFoundError(f"Chromosome sizes file not found: {chrom_sizes_file}")
            sizes = _rt.get_chroms_and_sizes(chrom_sizes_file)
            if chromosome not in sizes:
                raise ValueError(f"Chromosome {chromosome} not found in chromosome sizes file: {chrom_sizes_file}")
            chrom_size = int(sizes[chromosome])
            metadata = _get_bam_count_metadata(bam_file, step=step, norm_method=norm_method, effective_genome_size=effective_genome_size,
                                               ignore_for_norm=ignore_for_norm, flag_exclude=flag_exclude, extend_reads=extend_reads,
                                               num_processors=threads, scale_factor=scale_factor)
            file = _cached_file(bam_file)
            if chromosome not in file.records:
                logger.warning("Chromosome %s not found in BAM file: %s. Returning (None,None).", chromosome, bam_file)
            else:
                present.append(k)
                records_list.append(file.records[chromosome])
                metadata_list.append(metadata)
            before[k], held.records = held.records, []
    except BaseException:
        logger.removeFilter(held)
        for record in [r for records in before for r in records] + held.records:
            logger.handle(record)  # (an error cut the call short: what was logged up to it is not lost)
        raise
    logger.removeFilter(held)
    names = [input_files[k] for k in present]
    starts, matrix, file_logs, has_data = _rt._bam_matrix_batch(records_list, chrom_size, step, metadata_list, min_mapping_score,
                                                                flag_include, flag_exclude, center_reads, const_scale, round_digits,
                                                                scale_by_step, low_memory, names, chromosome)
    after = dict(zip(present, file_logs))
    live = dict(zip(present, has_data))
    for k in range(K):
        for record in before[k]:
            logger.handle(record)
        _rt._emit(after.get(k, ()))
    _rt._emit(_rt._excluded_records(input_files, [live.get(k, False) for k in range(K)], chromosome))
    return starts, matrix


def generate_chrom_matrix(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, const_scale: float = 1.0,
                          round_digits: int = 5, scale_by_step: bool = False, effective_genome_size: float = -1,
                          norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                          extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                          num_processors: int = -1, low_memory: bool = False):
    """`generate_chrom_matrix_device` with the reference's signature and return value (rocco/readtracks.py:521-633): NumPy
    ``(common_intervals.astype(int), count_matrix)``, or ``(None, None)``."""
    starts, matrix = generate_chrom_matrix_device(chromosome, input_files, chrom_sizes_file, step, const_scale, round_digits, scale_by_step,
                                                  effective_genome_size, norm_method, min_mapping_score, flag_include, flag_exclude,
                                                  extend_reads, center_reads, ignore_for_norm, scale_factor, num_processors, low_memory)
    if starts is None:
        return None, None
    return starts.astype(int), matrix.cpu().numpy()
