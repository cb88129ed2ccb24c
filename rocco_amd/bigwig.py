"""Read the data blocks of bigWig files without pyBigWig (note (31)): the container is walked on
the host (the 64-byte header, the chromosome B+ tree, the R-tree index down to the data blocks of one chromosome), the data
blocks of one or many files go up as ONE block table with their compressed bytes and are inflated on the device
(``inflate="device"``, the default: csrc/bgzf_inflate.hip's decoder under zlib framing, one wavefront per block, header
check and Adler-32 in HIP) or on the host (``inflate="host"``: `zlib.decompress` on a thread pool, test support).  What comes
out are the inflated sections in HBM, one slot per block in R-tree leaf order -- the order libBigWig's
``bwGetOverlappingIntervals`` reads them in.

Not built: the decode of the sections into (start, end, value) intervals on the device, and with it the reference's
``get_bigwig_chrom_scores`` / ``generate_chrom_matrix`` over bigWig paths (note (31) says why); zoom levels (never read, as
``intervals()`` never reads them), big-endian files (refused), bigBed."""
from __future__ import annotations

import collections
import os
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import dp as _dp
from .inflate import (  # noqa: F401  (what the BAM reader shares; the zlib names stay importable from here)
    BGZF_ERR_LENGTH, BGZF_ERR_STREAM, BGZF_MAX_ISIZE, ZLIB_ERR_ADLER, ZLIB_ERR_HEADER, ZLIB_ERR_TRUNCATED, ZLIB_HEADER_REASONS, ZLIB_MAX_GRID,
    ZLIB_TABLE_COLUMNS, _ADLER_TEXT, _HEADER_REASON_TEXT, _STREAM_REASON_TEXT, _TRUNCATED_TEXT, SpanList, _host_buffer, on_pool, upload_blocks,
    zlib_inflate_blocks_device, zlib_inflate_blocks_host, zlib_shape)

DEFAULT_INFLATE = "device"  # where the data blocks are inflated: "device" or "host"

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
