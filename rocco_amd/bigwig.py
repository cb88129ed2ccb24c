"""Read the data blocks of bigWig files without pyBigWig (note (31)): the container is walked on
the host (the 64-byte header, the chromosome B+ tree, the R-tree index down to the data blocks of one chromosome), the data
blocks of one or many files go up as ONE block table with their compressed bytes and are inflated on the device
(``inflate="device"``, the default: csrc/bgzf_inflate.hip's decoder under zlib framing, one wavefront per block, header
check and Adler-32 in HIP) or on the host (``inflate="host"``: `zlib.decompress` on a thread pool, test support).  What comes
out are the inflated sections in HBM, one slot per block in R-tree leaf order -- the order libBigWig's
``bwGetOverlappingIntervals`` reads them in.

The sections are decoded where they lie (csrc/bigwig_sections.hip over the rules of csrc/bigwig_sections.h, which the host
twin `decode_sections_host` compiles too): `read_bigwig_intervals` / `read_bigwig_intervals_batch` return what pyBigWig's
``intervals(chromosome)`` lists as three CUDA tensors, `get_bigwig_chrom_scores` and `generate_chrom_matrix(_device)` are the
reference's functions of these names over bigWig paths (rocco/readtracks.py:94-186, 521-633) with no pyBigWig behind them.

Not built: zoom levels (never read, as ``intervals()`` never reads them), big-endian files (refused), bigBed, a dense fill
over several files at once."""
from __future__ import annotations

import collections
import ctypes
import logging
import os
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import dp as _dp
from . import readtracks as _rt
from .inflate import (  # noqa: F401  (what the BAM reader shares; the zlib names stay importable from here)
    BGZF_ERR_LENGTH, BGZF_ERR_STREAM, BGZF_MAX_ISIZE, ZLIB_ERR_ADLER, ZLIB_ERR_HEADER, ZLIB_ERR_TRUNCATED, ZLIB_HEADER_REASONS, ZLIB_MAX_GRID,
    ZLIB_TABLE_COLUMNS, _ADLER_TEXT, _HEADER_REASON_TEXT, _STREAM_REASON_TEXT, _TRUNCATED_TEXT, SpanList, _host_buffer, on_pool, upload_blocks,
    zlib_inflate_blocks_device, zlib_inflate_blocks_host, zlib_shape)

DEFAULT_INFLATE = "device"  # where the data blocks are inflated: "device" or "host"
logger = logging.getLogger(__name__)

# ROCCO_BIGWIG_* of include/rocco_hip.h
BIGWIG_ERR_SHORT, BIGWIG_ERR_TYPE, BIGWIG_ERR_ITEMS, BIGWIG_ERR_WRAP = 8, 9, 10, 11
SECTION_HEADER_BYTES, SECTION_MAX_END = 24, 0xFFFFFFFF
_SECTION_TEXT = {
    BIGWIG_ERR_SHORT: f"the section is shorter than its {SECTION_HEADER_BYTES}-byte header",
    BIGWIG_ERR_TYPE: "the section's type is not 1 (bedGraph), 2 (variableStep) or 3 (fixedStep)",
    BIGWIG_ERR_ITEMS: "the section's header counts more items than its bytes hold (libBigWig would read past the section)",
    BIGWIG_ERR_WRAP: f"an item of the section ends beyond {SECTION_MAX_END} (libBigWig would wrap around)",
}

BIGWIG_MAGIC, CHROM_TREE_MAGIC, RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
_HEADER, _ZOOM_HEADER, _CHROM_TREE_HEADER, _RTREE_HEADER, _NODE_HEADER = 64, 24, 32, 48, 4
_RTREE_LEAF = np.dtype([("start_chrom", "<u4"), ("start_base", "<u4"), ("end_chrom", "<u4"), ("end_base", "<u4"), ("offset", "<u8"), ("size", "<u8")])
_RTREE_CHILD = np.dtype([("start_chrom", "<u4"), ("start_base", "<u4"), ("end_chrom", "<u4"), ("end_base", "<u4"), ("offset", "<u8")])
MAX_TREE_DEPTH = 64


# --------------------------------------------------------------------------------------------
# host: the container
# --------------------------------------------------------------------------------------------

class BigWigFile:
    """What `open_bigwig` keeps of a file: ``header`` (the fields of the 64-byte header), ``zooms`` (the zoom headers, never
    followed), ``chroms`` ({name: (id, length)}), ``size``, and per chromosome id the R-tree leaves once asked for."""

    def __init__(self, name: str, size: int, header: dict, zooms: list, chroms: dict):
        self.name, self.size, self.header, self.zooms, self.chroms = name, size, header, zooms, chroms
        self.leaves: dict = {}

    def chrom_lengths(self) -> dict:
        """pyBigWig's ``bw.chroms()``."""
        return {name: length for name, (_, length) in self.chroms.items()}


def _raw(path: str) -> np.ndarray:
    """The file's bytes, mapped (read once where they are used)."""
    if os.path.getsize(path) == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r")


def _bad(name: str, what: str, at: int, why: str) -> ValueError:
    return ValueError(f"{name}: {what} at file offset {at}: {why}")


def _need(raw, name: str, what: str, at: int, n: int) -> None:
    if at < 0 or n < 0 or at + n > len(raw):
        raise _bad(name, what, at, f"{n} bytes from there leave the file ({len(raw)} bytes)")


def _parse_header(raw, name: str) -> Tuple[dict, list]:
    if len(raw) < 4:
        raise RuntimeError(f"Could not open bigWig file: {name}...try installing `pyBigWig`: `python -m pip install pybigwig`")
    (magic,) = struct.unpack_from("<I", raw, 0)
    if magic == struct.unpack("<I", struct.pack(">I", BIGWIG_MAGIC))[0]:
        raise _bad(name, "the header", 0, "byte-swapped magic: a big-endian bigWig file, which is not read")
    if magic != BIGWIG_MAGIC:
        raise RuntimeError(f"Could not open bigWig file: {name}...try installing `pyBigWig`: `python -m pip install pybigwig`")
    _need(raw, name, "the header", 0, _HEADER)
    keys = ("magic", "version", "zoomLevels", "chromosomeTreeOffset", "fullDataOffset", "fullIndexOffset", "fieldCount", "definedFieldCount",
            "autoSqlOffset", "totalSummaryOffset", "uncompressBufSize", "extensionOffset")
    header = dict(zip(keys, struct.unpack_from("<IHHQQQHHQQIQ", raw, 0)))
    _need(raw, name, "the zoom headers", _HEADER, _ZOOM_HEADER * header["zoomLevels"])
    zooms = [dict(zip(("reductionLevel", "reserved", "dataOffset", "indexOffset"), struct.unpack_from("<IIQQ", raw, _HEADER + _ZOOM_HEADER * k)))
             for k in range(header["zoomLevels"])]
    return header, zooms


def _parse_chrom_tree(raw, name: str, at: int) -> dict:
    """{chromosome: (id, length)} from the B+ tree at `at`, in tree order."""
    what = "the chromosome tree"
    _need(raw, name, what, at, _CHROM_TREE_HEADER)
    magic, _, key_size, val_size, _, _ = struct.unpack_from("<IIIIQQ", raw, at)
    if magic != CHROM_TREE_MAGIC:
        raise _bad(name, what, at, f"magic {magic:#x} where {CHROM_TREE_MAGIC:#x} belongs")
    if val_size != 8 or key_size < 1:
        raise _bad(name, what, at, f"key size {key_size} and value size {val_size} (a bigWig file has values of 8 bytes)")
    chroms: dict = {}

    def walk(node: int, depth: int) -> None:
        if depth > MAX_TREE_DEPTH:
            raise _bad(name, what, node, f"the tree nests deeper than {MAX_TREE_DEPTH} levels")
        _need(raw, name, what, node, _NODE_HEADER)
        is_leaf, _, count = struct.unpack_from("<BBH", raw, node)
        item = key_size + 8
        _need(raw, name, what, node + _NODE_HEADER, count * item)
        for k in range(count):
            entry = node + _NODE_HEADER + k * item
            if is_leaf:
                key = bytes(raw[entry: entry + key_size]).split(b"\0", 1)[0].decode("latin-1")
                chroms[key] = struct.unpack_from("<II", raw, entry + key_size)
            else:
                (child,) = struct.unpack_from("<Q", raw, entry + key_size)
                if child <= node:
                    raise _bad(name, what, node, f"child offset {child} does not advance")
                walk(child, depth + 1)

    walk(at + _CHROM_TREE_HEADER, 1)
    return chroms


def _overlaps(items, leaf: bool, chrom_id: int, start: int, end: int) -> np.ndarray:
    """libBigWig's overlapsLeaf / overlapsNonLeaf (the lexicographic test on (chromosome, base)) over a node's items."""
    sc, sb, ec, eb = (items[f].astype(np.int64) for f in ("start_chrom", "start_base", "end_chrom", "end_base"))
    inside = (chrom_id >= sc) & (chrom_id <= ec)
    one = sc == ec
    ok_one = ~((sb >= end) | (eb <= start))
    ok_many = ~(((chrom_id == sc) & (sb >= end)) | ((chrom_id != sc) & (chrom_id == ec) & (eb <= start)))
    return inside & np.where(one, ok_one, ok_many)


def _rtree_leaves(raw, name: str, at: int, chrom_id: int, length: int) -> List[Tuple[int, int]]:
    """(dataOffset, dataSize) of the leaf items that overlap [0, length) of chromosome `chrom_id`, in tree order."""
    what = "the R-tree index"
    _need(raw, name, what, at, _RTREE_HEADER)
    (magic,) = struct.unpack_from("<I", raw, at)
    if magic != RTREE_MAGIC:
        raise _bad(name, what, at, f"magic {magic:#x} where {RTREE_MAGIC:#x} belongs")
    out: List[Tuple[int, int]] = []

    def walk(node: int, depth: int) -> None:
        if depth > MAX_TREE_DEPTH:
            raise _bad(name, what, node, f"the tree nests deeper than {MAX_TREE_DEPTH} levels")
        _need(raw, name, what, node, _NODE_HEADER)
        is_leaf, _, count = struct.unpack_from("<BBH", raw, node)
        dtype = _RTREE_LEAF if is_leaf else _RTREE_CHILD
        _need(raw, name, what, node + _NODE_HEADER, count * dtype.itemsize)
        items = np.frombuffer(raw, dtype=dtype, count=count, offset=node + _NODE_HEADER)
        for k in np.nonzero(_overlaps(items, bool(is_leaf), chrom_id, 0, length))[0].tolist():
            offset = int(items["offset"][k])
            if is_leaf:
                size = int(items["size"][k])
                if offset + size > len(raw):
                    raise _bad(name, f"data block {len(out)} (R-tree leaf at file offset {node})", offset,
                               f"{size} bytes from there leave the file ({len(raw)} bytes)")
                out.append((offset, size))
            else:
                if offset <= node:
                    raise _bad(name, what, node, f"child offset {offset} does not advance")
                walk(offset, depth + 1)

    walk(at + _RTREE_HEADER, 1)
    return out


_BIGWIG_CACHE: "collections.OrderedDict" = collections.OrderedDict()
BIGWIG_CACHE_FILES = 1024


def clear_bigwig_cache() -> None:
    """Drops every parsed header, chromosome dict and R-tree leaf list."""
    _BIGWIG_CACHE.clear()


def open_bigwig(path) -> BigWigFile:
    """The parsed container of a file, from the cache keyed on (path, size, mtime) or read now.  RuntimeError with the
    reference's words where the file is no bigWig file at all; ValueError naming the file, the structure and the file
    offset for everything else that is refused."""
    path = os.fspath(path)
    stat = os.stat(path)
    key = (os.path.abspath(path), int(stat.st_size), int(stat.st_mtime_ns))
    hit = _BIGWIG_CACHE.get(key)
    if hit is not None:
        _BIGWIG_CACHE.move_to_end(key)
        return hit
    raw = _raw(path)
    header, zooms = _parse_header(raw, path)
    file = BigWigFile(path, len(raw), header, zooms, _parse_chrom_tree(raw, path, header["chromosomeTreeOffset"]))
    _BIGWIG_CACHE[key] = file
    while len(_BIGWIG_CACHE) > BIGWIG_CACHE_FILES:
        _BIGWIG_CACHE.popitem(last=False)
    return file


def chrom_blocks(file: BigWigFile, chromosome: str, raw=None) -> List[Tuple[int, int]]:
    """(dataOffset, dataSize) of the chromosome's data blocks in R-tree leaf order (the order libBigWig reads them in)."""
    chrom_id, length = file.chroms[chromosome]
    if chrom_id not in file.leaves:
        raw = _raw(file.name) if raw is None else raw
        file.leaves[chrom_id] = _rtree_leaves(raw, file.name, file.header["fullIndexOffset"], chrom_id, length)
    return file.leaves[chrom_id]


# --------------------------------------------------------------------------------------------
# the block table, the two inflates
# --------------------------------------------------------------------------------------------

def slot_stride(capacity: int) -> int:
    return (int(capacity) + 7) // 8 * 8


def _status_words(status: int, produced: int, capacity: int) -> str:
    code, why = status & 0xFF, status >> 8
    if code == BGZF_ERR_STREAM:
        return f"the zlib stream does not inflate ({_STREAM_REASON_TEXT.get(why, f'reason {why}')})"
    if code == ZLIB_ERR_HEADER:
        return f"the zlib stream does not inflate ({_HEADER_REASON_TEXT.get(why, f'header reason {why}')})"
    if code == ZLIB_ERR_TRUNCATED:
        return f"the zlib stream does not inflate ({_TRUNCATED_TEXT})"
    if code == ZLIB_ERR_ADLER:
        return f"the zlib stream does not inflate ({_ADLER_TEXT})"
    if code == BGZF_ERR_LENGTH:
        return f"length mismatch (the file's uncompressBufSize is {capacity}, the data inflates to {produced})"
    return f"its row of the block table does not fit the buffers (status {status})"


def host_block_status(span: bytes, capacity: int, framing: int = 0) -> Tuple[int, bytes]:
    """(status, bytes) of one block through `zlib.decompress`, in the status words and the precedence of
    `rocco_hip_zlib_inflate`: header, stream, truncated, length, Adler-32."""
    if framing == 1:
        return (BGZF_ERR_LENGTH if len(span) > capacity else 0), bytes(span)
    try:
        data = zlib.decompress(span)
    except zlib.error as exc:
        text = str(exc)
        words = text[text.index("data: ") + 6:] if "data: " in text else ""
        for why, said in _HEADER_REASON_TEXT.items():
            if words == said:
                return ZLIB_ERR_HEADER | why << 8, b""
        if text.startswith("Error 2 "):  # Z_NEED_DICT
            return ZLIB_ERR_HEADER | 4 << 8, b""
        for why, said in _STREAM_REASON_TEXT.items():
            if words == said and why != 12:
                return BGZF_ERR_STREAM | why << 8, b""
        if words == _TRUNCATED_TEXT and (len(span) < 2 or span[1] & 0x20):  # (no header, or no dictionary id behind FDICT)
            return ZLIB_ERR_TRUNCATED, b""
        body = zlib.decompressobj(wbits=-15)
        data = body.decompress(span[2:])
        if words == _TRUNCATED_TEXT:  # (inside the deflate data: a stream error; behind it: no room for the check value)
            return (ZLIB_ERR_TRUNCATED if body.eof else BGZF_ERR_STREAM | 12 << 8), (data if body.eof else b"")
        if words == _ADLER_TEXT:
            return (BGZF_ERR_LENGTH if len(data) > capacity else ZLIB_ERR_ADLER), data
        raise
    return (BGZF_ERR_LENGTH if len(data) > capacity else 0), data


def _resolve_inflate(inflate: Optional[str]) -> str:
    inflate = DEFAULT_INFLATE if inflate is None else inflate
    if inflate not in ("device", "host"):
        raise ValueError(f"inflate must be \"device\" or \"host\", not {inflate!r}")
    return inflate


def _block_where(name: str, index: int, at: int) -> str:
    return f"{name}: bigWig data block {index} at file offset {at}"


def _chrom_layout(wanted: Sequence[Tuple[BigWigFile, str]], inflate: str):
    """ONE block table and one compressed buffer for the data blocks of one chromosome of each of K files: (the table int64
    [n][5], the span list, per block its (file index, index among the chromosome's blocks, file offset), the K + 1 block
    offsets of the files, the bytes of the slots)."""
    blocks, file_first, spans, rows = [], [0], SpanList(), []
    for k, (file, chromosome) in enumerate(wanted):
        raw = _raw(file.name)  # (mapped: the span list tells the files apart by it)
        leaves = chrom_blocks(file, chromosome, raw)
        buf = int(file.header["uncompressBufSize"])
        framing = 0 if buf > 0 else 1
        capacity = buf if buf > 0 else max((size for _, size in leaves), default=0)
        if inflate == "device" and capacity > BGZF_MAX_ISIZE:
            raise _bad(file.name, "the header", 0, f"uncompressBufSize {capacity} exceeds {BGZF_MAX_ISIZE}: the device inflate holds no larger "
                       "block and no CPU fallback exists for such blocks in device mode (inflate=\"host\" reads this file)")
        for index, (offset, size) in enumerate(leaves):
            # (the blocks of a chromosome lie one behind the other in files written by the usual tools: they ride in one span)
            comp_at = spans.add(raw, offset, offset + size)
            rows.append((comp_at, comp_at + size, capacity, framing))
            blocks.append((k, index, offset))
        file_first.append(len(rows))
    table = np.zeros((len(rows), ZLIB_TABLE_COLUMNS), dtype=np.int64)
    if rows:
        table[:, [0, 1, 2, 4]] = np.asarray(rows, dtype=np.int64)
        strides = (table[:, 2] + 7) // 8 * 8
        table[1:, 3] = np.cumsum(strides[:-1])
    n_out = int(table[-1, 3] + (table[-1, 2] + 7) // 8 * 8) if rows else 0
    return table, spans, blocks, np.asarray(file_first, dtype=np.int64), n_out


def inflate_chrom_blocks(wanted: Sequence[Tuple[BigWigFile, str]], dev, inflate: str):
    """The inflated data blocks of one chromosome of each of K files: the one table of `_chrom_layout`, one upload, one
    inflate.  Returns (slots uint8 CUDA tensor, the block table int64 CUDA tensor [n][5], produced int64 CUDA tensor [n],
    the K + 1 block offsets of the files): block i's bytes are ``slots[table[i, 3]: table[i, 3] + produced[i]]``."""
    import torch

    table, spans, blocks, file_first, n_out = _chrom_layout(wanted, inflate)

    def refuse(block: int, words: str) -> ValueError:
        k, index, offset = blocks[block]
        return ValueError(f"{_block_where(wanted[k][0].name, index, offset)}: {words}")

    with torch.cuda.device(dev):
        if inflate == "device":
            table_t, comp_t = upload_blocks(table, spans.spans, spans.n_comp, dev)
            slots_t = torch.empty(n_out, dtype=torch.uint8, device=dev)
            _, produced_t, report = zlib_inflate_blocks_device(comp_t, table_t, slots_t)  # (synchronises: the upload's pinned buffer may go)
            if report["block"] >= 0:
                raise refuse(report["block"], _status_words(report["status"], report["produced"], int(table[report["block"], 2])))
        else:
            slots = _host_buffer(n_out)
            raws = [_raw(file.name) for file, _ in wanted]

            def one(i):
                lo, hi, capacity, slot, framing = (int(v) for v in table[i])
                k, _, offset = blocks[i]
                status, data = host_block_status(raws[k][offset: offset + hi - lo].tobytes(), capacity, framing)
                if status == 0:
                    slots[slot: slot + len(data)] = np.frombuffer(data, dtype=np.uint8)
                return status, len(data)

            done = on_pool(one, range(table.shape[0]))
            produced = np.asarray([n for _, n in done], dtype=np.int64).reshape(-1)
            for i, (status, n) in enumerate(done):
                if status != 0:
                    raise refuse(i, _status_words(status, n, int(table[i, 2])))
            slots_t = torch.from_numpy(slots).to(dev)
            table_t = torch.from_numpy(table.reshape(-1)).to(dev)
            produced_t = torch.from_numpy(produced).to(dev)
    return slots_t, table_t.view(-1, ZLIB_TABLE_COLUMNS), produced_t, file_first


# --------------------------------------------------------------------------------------------
# the Python API
# --------------------------------------------------------------------------------------------

def read_bigwig_blocks(path, chromosome: str, device=None, inflate: Optional[str] = None):
    """The inflated data blocks of a chromosome, in R-tree leaf order (the order libBigWig reads them in): (slots uint8,
    block table int64 [n][5], produced int64 [n]) as CUDA tensors; block i's section is
    ``slots[table[i, 3]: table[i, 3] + produced[i]]``.  KeyError where the file does not have the chromosome; ValueError
    naming the file, the block and its file offset, with zlib's words, for a block that does not inflate.  ``inflate``:
    "device" (`DEFAULT_INFLATE`) or "host"."""
    inflate = _resolve_inflate(inflate)
    dev = _dp._device(device)
    file = open_bigwig(path)
    if chromosome not in file.chroms:
        raise KeyError(f"{file.name}: no chromosome {chromosome}")
    slots, table, produced, _ = inflate_chrom_blocks([(file, chromosome)], dev, inflate)
    return slots, table, produced


# --------------------------------------------------------------------------------------------
# the sections -> intervals (csrc/bigwig_sections.h, csrc/bigwig_sections.hip)
# --------------------------------------------------------------------------------------------

def sections_shape() -> dict:
    """`rocco_hip_bigwig_sections_shape`: the lanes per block, the grid cap, the bytes of a section's header."""
    shape = (ctypes.c_int * 3)()
    _native.load().rocco_hip_bigwig_sections_shape(shape)
    return dict(zip(("threads", "max_grid", "header_bytes"), (int(v) for v in shape)))


def _file_arrays(file_first, chrom_ids, chrom_lengths):
    """The three host arrays of the section entry points, int64: K + 1 block offsets, K chromosome ids, K chromosome lengths."""
    first, ids, lengths = (np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64) for a in (file_first, chrom_ids, chrom_lengths))
    if first.size != ids.size + 1 or ids.size != lengths.size:
        raise ValueError("K + 1 block offsets, K chromosome ids and K chromosome lengths are required")
    return first, ids, lengths


def _ll(a: np.ndarray):
    return a.ctypes.data_as(_native.c_ll_p)


def decode_sections_host(slots, table, produced, file_first, chrom_ids, chrom_lengths, emit: bool = True) -> dict:
    """`rocco_hip_bigwig_sections_host` (test support: the kernels' rules compiled for the host, on the calling thread) over
    NumPy arrays: ``status`` int32 per block, ``block_first`` int64 [n + 1], ``file_offsets`` int64 [K + 1], ``report``
    (``block`` / ``status`` / ``produced``: the total), and with ``emit`` where no block is refused ``starts`` / ``ends``
    int64 and ``values`` float64 (else None)."""
    slots = np.ascontiguousarray(slots, dtype=np.uint8).reshape(-1)
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, ZLIB_TABLE_COLUMNS)
    produced = np.ascontiguousarray(produced, dtype=np.int64).reshape(-1)
    first, ids, lengths = _file_arrays(file_first, chrom_ids, chrom_lengths)
    n = table.shape[0]
    if produced.size != n:
        raise ValueError("one produced per row of the block table is required")
    status, block_first = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
    offsets, back = np.zeros(first.size, dtype=np.int64), (ctypes.c_longlong * 4)()

    def ptr(a):
        return a.ctypes.data if a is not None and a.size else None

    def call(starts, ends, values):
        _native.check(_native.load().rocco_hip_bigwig_sections_host(
            None, ptr(slots), slots.size, ptr(table), ptr(produced), n, _ll(first), _ll(ids), _ll(lengths), ids.size, ptr(status), n,
            block_first.ctypes.data, block_first.size, _ll(offsets), ptr(starts), 0 if starts is None else starts.size, ptr(ends),
            0 if ends is None else ends.size, ptr(values), 0 if values is None else values.size, back), "rocco_hip_bigwig_sections_host")

    call(None, None, None)
    out = {"status": status, "block_first": block_first, "file_offsets": offsets, "report": _report(back), "starts": None, "ends": None,
           "values": None}
    if emit and back[0] < 0:
        total = int(back[2])
        starts, ends, values = np.empty(total, dtype=np.int64), np.empty(total, dtype=np.int64), np.empty(total, dtype=np.float64)
        if total:
            call(starts, ends, values)
        out.update(starts=starts, ends=ends, values=values)
    return out


def _report(back) -> dict:
    return {"block": int(back[0]), "status": int(back[1]), "produced": int(back[2])}


def _section_inputs(slots_t, table_t, produced_t):
    import torch

    for t, dtype in ((slots_t, torch.uint8), (table_t, torch.int64), (produced_t, torch.int64)):
        if not _dp._is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.device != slots_t.device:
            raise TypeError("the sections: contiguous CUDA tensors on one device are required (uint8, int64, int64)")
    if table_t.numel() % ZLIB_TABLE_COLUMNS or table_t.numel() // ZLIB_TABLE_COLUMNS != produced_t.numel():
        raise ValueError(f"the block table has {ZLIB_TABLE_COLUMNS} columns and one produced per row")
    return produced_t.numel()


def sections_facts_device(slots_t, table_t, produced_t, file_first, chrom_ids, chrom_lengths):
    """`rocco_hip_bigwig_sections_facts` over what `inflate_chrom_blocks` returns: (int32 status per block, int64 block_first
    [n + 1] -- both CUDA tensors --, the K + 1 interval offsets of the files as a NumPy array, the report).  Returns when the
    kernels have run."""
    import torch

    n = _section_inputs(slots_t, table_t, produced_t)
    first, ids, lengths = _file_arrays(file_first, chrom_ids, chrom_lengths)
    dev = slots_t.device
    status_t = torch.empty(n, dtype=torch.int32, device=dev)
    block_first_t = torch.empty(n + 1, dtype=torch.int64, device=dev)
    offsets, back = np.zeros(first.size, dtype=np.int64), (ctypes.c_longlong * 4)()
    with torch.cuda.device(dev):
        _native.check(_native.load().rocco_hip_bigwig_sections_facts(
            _native.solver_for(dev.index).handle, slots_t.data_ptr() or None, slots_t.numel(), table_t.data_ptr() or None,
            produced_t.data_ptr() or None, n, _ll(first), _ll(ids), _ll(lengths), ids.size, status_t.data_ptr() or None, n,
            block_first_t.data_ptr(), n + 1, _ll(offsets), back, _dp._stream_ptr(slots_t)), "rocco_hip_bigwig_sections_facts")
    return status_t, block_first_t, offsets, _report(back)


def sections_emit_device(slots_t, table_t, produced_t, file_first, chrom_ids, chrom_lengths, block_first_t, total: int, starts_t, ends_t,
                         values_t) -> None:
    """`rocco_hip_bigwig_sections_emit`: the ``total`` kept items into the first cells of ``starts_t`` / ``ends_t`` (int64) and
    ``values_t`` (float64), whose sizes go along.  Not called for a total of 0 (an empty tensor has no address)."""
    import torch

    n = _section_inputs(slots_t, table_t, produced_t)
    first, ids, lengths = _file_arrays(file_first, chrom_ids, chrom_lengths)
    dev = slots_t.device
    for t, dtype in ((block_first_t, torch.int64), (starts_t, torch.int64), (ends_t, torch.int64), (values_t, torch.float64)):
        if not _dp._is_tensor(t) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise TypeError("sections_emit_device: contiguous CUDA tensors on the sections' device are required (int64, int64, int64, float64)")
    if int(total) == 0:
        return
    with torch.cuda.device(dev):
        _native.check(_native.load().rocco_hip_bigwig_sections_emit(
            _native.solver_for(dev.index).handle, slots_t.data_ptr() or None, slots_t.numel(), table_t.data_ptr() or None,
            produced_t.data_ptr() or None, n, _ll(first), _ll(ids), _ll(lengths), ids.size, block_first_t.data_ptr() or None,
            block_first_t.numel(), int(total), starts_t.data_ptr() or None, starts_t.numel(), ends_t.data_ptr() or None, ends_t.numel(),
            values_t.data_ptr() or None, values_t.numel(), _dp._stream_ptr(slots_t)), "rocco_hip_bigwig_sections_emit")


def decode_sections_device(slots_t, table_t, produced_t, file_first, chrom_ids, chrom_lengths) -> dict:
    """Both calls: ``status`` (CUDA int32), ``file_offsets`` (NumPy, K + 1), ``report``, and where no block is refused
    ``starts`` / ``ends`` (CUDA int64) and ``values`` (CUDA float64), else None.  No block: no call."""
    import torch

    dev = slots_t.device
    n = _section_inputs(slots_t, table_t, produced_t)
    first, ids, lengths = _file_arrays(file_first, chrom_ids, chrom_lengths)
    if n == 0:
        status_t, offsets, report, block_first_t = torch.empty(0, dtype=torch.int32, device=dev), np.zeros(first.size, dtype=np.int64), _report((-1, 0, 0)), None
    else:
        status_t, block_first_t, offsets, report = sections_facts_device(slots_t, table_t, produced_t, first, ids, lengths)
    out = {"status": status_t, "file_offsets": offsets, "report": report, "starts": None, "ends": None, "values": None}
    if report["block"] < 0:
        total = report["produced"]
        starts_t, ends_t = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int64, device=dev)
        values_t = torch.empty(total, dtype=torch.float64, device=dev)
        if total:
            sections_emit_device(slots_t, table_t, produced_t, first, ids, lengths, block_first_t, total, starts_t, ends_t, values_t)
        out.update(starts=starts_t, ends=ends_t, values=values_t)
    return out


def _section_words(status: int) -> str:
    return _SECTION_TEXT.get(status & 0xFF, f"its row of the block table does not fit the buffers (status {status})")


def read_bigwig_intervals_batch(wanted: Sequence[Tuple[str, str]], device=None, inflate: Optional[str] = None) -> list:
    """For every (path, chromosome): what pyBigWig's ``intervals(chromosome)`` lists, as (starts int64, ends int64, values
    float64) CUDA tensors in its order -- views into three arrays that hold the intervals of all files --, or None for a
    chromosome the file lacks.  One block table, one inflate and one decode for all files (two waits for the device in the
    decode, one in the device inflate).  ValueError naming the file, the block and its file offset for a block that does
    not inflate or whose section is refused (csrc/bigwig_sections.h says what libBigWig would have done with it)."""
    inflate = _resolve_inflate(inflate)
    dev = _dp._device(device)
    files = [open_bigwig(path) for path, _ in wanted]
    present = [k for k, (file, (_, chromosome)) in enumerate(zip(files, wanted)) if chromosome in file.chroms]
    out: list = [None] * len(wanted)
    if not present:
        return out
    pairs = [(files[k], wanted[k][1]) for k in present]
    slots, table, produced, file_first = inflate_chrom_blocks(pairs, dev, inflate)
    ids = [file.chroms[chromosome][0] for file, chromosome in pairs]
    lengths = [file.chroms[chromosome][1] for file, chromosome in pairs]
    got = decode_sections_device(slots, table.reshape(-1), produced, file_first, ids, lengths)
    if got["report"]["block"] >= 0:
        block = got["report"]["block"]
        k = int(np.searchsorted(file_first, block, side="right")) - 1
        index = block - int(file_first[k])
        file, chromosome = pairs[k]
        raise ValueError(f"{_block_where(file.name, index, chrom_blocks(file, chromosome)[index][0])}: {_section_words(got['report']['status'])}")
    offsets = got["file_offsets"]
    for j, k in enumerate(present):
        lo, hi = int(offsets[j]), int(offsets[j + 1])
        out[k] = (got["starts"][lo:hi], got["ends"][lo:hi], got["values"][lo:hi])
    return out


def read_bigwig_intervals(path, chromosome: str, device=None, inflate: Optional[str] = None):
    """What pyBigWig's ``open(path).intervals(chromosome)`` lists, as (starts int64, ends int64, values float64) CUDA tensors
    in its order (the values are the file's float32 widened), or None for a chromosome the file lacks.  A chromosome without
    intervals gives three empty tensors (pyBigWig: None).  Errors as `read_bigwig_intervals_batch`."""
    return read_bigwig_intervals_batch([(os.fspath(path), chromosome)], device=device, inflate=inflate)[0]


# --------------------------------------------------------------------------------------------
# the reference's two entry points over bigWig paths (rocco/readtracks.py:94-186, 521-633)
# --------------------------------------------------------------------------------------------

def _checked_open(bigwig_file: str, chromosome: str, chrom_sizes_file: str) -> BigWigFile:
    """What the reference's ``get_bigwig_chrom_scores`` does before it asks for intervals, in its order
    (rocco/readtracks.py:103-119)."""
    if not os.path.exists(bigwig_file):
        raise FileNotFoundError(f"bigWig file not found: {bigwig_file}")
    if not os.path.exists(chrom_sizes_file):
        raise FileNotFoundError(f"Chromosome sizes file not found: {chrom_sizes_file}")
    if chromosome not in _rt.get_chroms_and_sizes(chrom_sizes_file):
        raise ValueError(f"Chromosome {chromosome} not found in chromosome sizes file: {chrom_sizes_file}")
    return open_bigwig(bigwig_file)


def _scores_of(bigwig_file: str, chromosome: str, file: BigWigFile, intervals, const_scale: float, round_digits: int, dev):
    """rocco/readtracks.py:121-186 for a file already open and read: (first start, step, values in HBM) or (None, None, None),
    with the reference's warnings and errors in its order."""
    if chromosome not in file.chroms:
        logger.warning("Chromosome %s not found in bigWig file: %s. Returning (None,None).", chromosome, bigwig_file)
        return None, None, None
    starts, ends, values = intervals
    if int(starts.shape[0]) == 0:
        logger.warning("No intervals found in bigWig file: %s for chromosome: %s. Returning (None,None).", bigwig_file, chromosome)
        return None, None, None
    first, step, full = _rt.bigwig_dense_fill_device(starts, ends, values, const_scale=const_scale, round_digits=round_digits,
                                                     bigwig_file=bigwig_file, chromosome=chromosome, device=dev)
    if const_scale == 0:  # (behind the five validations, where the reference has it)
        logger.warning("You are scaling the values by 0.")
    return first, step, full


def get_bigwig_chrom_scores_device(bigwig_file: str, chromosome: str, chrom_sizes_file: str, const_scale: float = 1.0, round_digits: int = 5,
                                   device=None, inflate: Optional[str] = None):
    """`get_bigwig_chrom_scores` with the track left in HBM: (first start, step, values as a float64 CUDA tensor), the
    reference's ``full_intervals`` being ``first + step * arange(len(values))``; (None, None, None) where it returns
    (None, None)."""
    file = _checked_open(bigwig_file, chromosome, chrom_sizes_file)
    dev = _dp._device(device)
    intervals = read_bigwig_intervals(bigwig_file, chromosome, device=dev, inflate=inflate) if chromosome in file.chroms else None
    return _scores_of(bigwig_file, chromosome, file, intervals, const_scale, round_digits, dev)


def get_bigwig_chrom_scores(bigwig_file: str, chromosome: str, chrom_sizes_file: str, const_scale: float = 1.0, round_digits: int = 5):
    """rocco/readtracks.py:94-186 with the same arguments, return value, errors and log records, and no pyBigWig: the container
    on the host, inflate, section decode, validation, dense fill, scaling and rounding on the device.  The binding:
    ``rocco_amd.readtracks.get_bigwig_chrom_scores = rocco_amd.bigwig.get_bigwig_chrom_scores``."""
    first, step, full = get_bigwig_chrom_scores_device(bigwig_file, chromosome, chrom_sizes_file, const_scale, round_digits)
    if first is None:
        return None, None
    return np.arange(first, first + step * int(full.shape[0]), step, dtype=np.int64).astype(int), full.cpu().numpy()


def generate_chrom_matrix_device(chromosome: str, input_files: list, chrom_sizes_file: str, step: int, const_scale: float = 1.0,
                                 round_digits: int = 5, scale_by_step: bool = False, effective_genome_size: float = -1,
                                 norm_method: str = "RPGC", min_mapping_score: int = 10, flag_include=None, flag_exclude: int = 3844,
                                 extend_reads: int = -1, center_reads: bool = False, ignore_for_norm=None, scale_factor: float = 1.0,
                                 num_processors: int = -1, low_memory: bool = False, device=None, inflate: Optional[str] = None):
    """The reference's ``generate_chrom_matrix`` over bigWig files (rocco/readtracks.py:521-633, same keywords; those of the BAM
    branch are taken and not used, as there) with the matrix left on the device: (starts as a host ``int`` array, matrix as a
    CUDA tensor), or ``(None, None)``.  The files are read in ONE batch (`read_bigwig_intervals_batch`), then filled one by
    one in file order, so errors and log records come as the reference's per-file loop gives them: a file the reference
    would not have reached (one behind the first that raises) is not looked at.  This is the function to bind behind
    ``rocco_amd.rocco.generate_chrom_matrix`` for bigWig inputs."""
    import torch

    track_types = {_rt._get_track_type(input_file) for input_file in input_files}
    if len(track_types) != 1:
        raise ValueError("All input files must share the same type.")
    if next(iter(track_types)) != "bigwig":
        raise ValueError("rocco_amd.bigwig.generate_chrom_matrix reads bigWig files: BAM inputs go through rocco_amd.bam.generate_chrom_matrix")
    dev = _dp._device(device)
    opened, stopped = [], None
    for input_file in input_files:  # (what the reference does per file before it reads: up to the first file that raises)
        try:
            opened.append(_checked_open(input_file, chromosome, chrom_sizes_file))
        except (OSError, ValueError, RuntimeError) as exc:
            stopped = exc
            break
    read = read_bigwig_intervals_batch([(file.name, chromosome) for file in opened], device=dev, inflate=inflate)
    results = [_scores_of(input_file, chromosome, file, intervals, const_scale, round_digits, dev)
               for input_file, file, intervals in zip(input_files, opened, read)]
    if stopped is not None:
        raise stopped
    interval_matrix, vals_matrix = [], []
    for input_file, (first, step_, full) in zip(input_files, results):
        if first is None:
            logger.warning(f"No data found for {input_file} in chromosome {chromosome}. Excluding this track for {chromosome}.")
            continue
        interval_matrix.append(first + step_ * torch.arange(int(full.shape[0]), dtype=torch.int64, device=dev))
        vals_matrix.append(full)
    if not interval_matrix:
        logger.warning(f"No data found in the files {str(input_files)} for chromosome {chromosome}. Returning (None,None).")
        return None, None
    common, matrix = _rt.assemble_chrom_matrix_device(interval_matrix, vals_matrix, track_type="bigwig", low_memory=low_memory,
                                                      chromosome=chromosome, device=dev)
    return common.cpu().numpy().astype(int), matrix


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
    return starts, matrix.cpu().numpy()
