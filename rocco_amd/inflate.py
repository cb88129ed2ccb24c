"""What the readers of BGZF blocks (rocco_amd/bam.py) and of zlib-framed bigWig data blocks (rocco_amd/bigwig.py) share around the
device inflate (csrc/bgzf_inflate.hip, csrc/inflate_core.h; DESIGN.md notes (29), (31), (32)): the constants and reason texts of
include/rocco_hip.h, the calls of the four ``rocco_hip_*_inflate*`` entry points, and the staging of an upload -- the block
table in front of the coalesced compressed spans in ONE pinned buffer, ONE asynchronous copy, views of it as table and bytes."""
from __future__ import annotations

import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np

from . import _native
from . import dp as _dp

# ROCCO_BGZF_* of include/rocco_hip.h
BGZF_THREADS, BGZF_TABLE_COLUMNS, BGZF_MAX_ISIZE, BGZF_STREAM_REASONS = 64, 5, 65536, 12
BGZF_ERR_STREAM, BGZF_ERR_LENGTH, BGZF_ERR_CRC, BGZF_ERR_TABLE = range(1, 5)
BGZF_MAX_GRID = 1 << 20  # workgroups of an inflate launch at most: block i + BGZF_MAX_GRID is the next turn of block i's workgroup
_STREAM_REASON_TEXT = {
    1: "invalid block type", 2: "invalid stored block lengths", 3: "too many length or distance symbols", 4: "invalid code lengths set",
    5: "invalid bit length repeat", 6: "invalid code -- missing end-of-block", 7: "invalid literal/lengths set", 8: "invalid distances set",
    9: "invalid literal/length code", 10: "invalid distance code", 11: "invalid distance too far back", 12: "incomplete or truncated stream",
}
# ROCCO_ZLIB_*
ZLIB_TABLE_COLUMNS, ZLIB_HEADER_REASONS, ZLIB_MAX_GRID = 5, 4, 1 << 16
ZLIB_ERR_HEADER, ZLIB_ERR_ADLER, ZLIB_ERR_TRUNCATED = 5, 6, 7
_HEADER_REASON_TEXT = {1: "incorrect header check", 2: "unknown compression method", 3: "invalid window size", 4: "a preset dictionary is asked for"}
_TRUNCATED_TEXT, _ADLER_TEXT = "incomplete or truncated stream", "incorrect data check"


# --------------------------------------------------------------------------------------------
# host memory and the thread pool of the host modes
# --------------------------------------------------------------------------------------------

def _default_threads() -> int:
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:  # (no affinity interface on this platform)
        return 1


def _host_buffer(n: int) -> np.ndarray:
    """n bytes of host memory as a uint8 array: pinned where a device is present (uploads from it run asynchronously)."""
    import torch

    t = torch.empty(max(int(n), 1), dtype=torch.uint8)
    if torch.cuda.is_available():
        try:
            t = t.pin_memory()
        except RuntimeError:  # (no pinned memory left: ordinary memory uploads as well, synchronously)
            pass
    return t.numpy()[: int(n)]


def on_pool(one, jobs, threads: Optional[int] = None) -> list:
    """``[one(job) for job in jobs]`` on a pool of ``threads`` threads (zlib releases the GIL; default `_default_threads`); the
    first job in order that raises, raises here."""
    with ThreadPoolExecutor(max_workers=_default_threads() if threads is None else max(1, int(threads))) as pool:
        return list(pool.map(one, jobs))


# --------------------------------------------------------------------------------------------
# the entry points
# --------------------------------------------------------------------------------------------

def bgzf_shape() -> dict:
    """`rocco_hip_bgzf_shape`: the lanes per block, the columns of the block table, the largest ISIZE, the stream reasons."""
    shape = (ctypes.c_int * 4)()
    _native.load().rocco_hip_bgzf_shape(shape)
    return {"threads": int(shape[0]), "table_columns": int(shape[1]), "max_isize": int(shape[2]), "stream_reasons": int(shape[3])}


def zlib_shape() -> dict:
    """`rocco_hip_zlib_shape`: the lanes per block, the columns of the block table, the largest capacity, the header reasons, the grid cap."""
    shape = (ctypes.c_int * 5)()
    _native.load().rocco_hip_zlib_shape(shape)
    return dict(zip(("threads", "table_columns", "max_capacity", "header_reasons", "max_grid"), (int(v) for v in shape)))


def bgzf_block_table(blocks, base: int = 0) -> np.ndarray:
    """The block table of `rocco_hip_bgzf_inflate` for `_bgzf_blocks` rows: int64 [n][5] = first byte of the deflate data
    (relative to ``base``), one past its last, ISIZE, CRC32, the prefix sum of ISIZE."""
    table = np.zeros((len(blocks), BGZF_TABLE_COLUMNS), dtype=np.int64)
    if blocks:
        rows = np.asarray(blocks, dtype=np.int64)
        table[:, 0], table[:, 1], table[:, 2], table[:, 3] = rows[:, 1] - base, rows[:, 2] - base, rows[:, 4], rows[:, 3]
        table[1:, 4] = np.cumsum(table[:-1, 2])
    return table


def _report(back) -> dict:
    return {"block": int(back[0]), "status": int(back[1]), "produced": int(back[2])}


def _blocks_host(who: str, entry: str, columns: int, with_produced: bool, comp, table: np.ndarray, out: np.ndarray):
    """``entry`` (a ``rocco_hip_*_inflate_host``) over host arrays: (int32 status per block, int64 produced per block or None, the report)."""
    comp = np.ascontiguousarray(np.frombuffer(comp, dtype=np.uint8) if not isinstance(comp, np.ndarray) else comp)
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, columns)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise TypeError(f"{who}: out must be a writable contiguous uint8 array")
    status = np.zeros(table.shape[0], dtype=np.int32)
    produced = np.zeros(table.shape[0], dtype=np.int64) if with_produced else None
    back = (ctypes.c_longlong * 4)()
    per_block = [a.ctypes.data if a.size else None for a in (status, produced) if a is not None]
    _native.check(getattr(_native.load(), entry)(
        None, comp.ctypes.data if comp.size else None, comp.size, table.ctypes.data if table.size else None, table.shape[0],
        out.ctypes.data if out.size else None, out.size, *per_block, back), entry)
    return status, produced, _report(back)


def _blocks_device(who: str, entry: str, columns: int, with_produced: bool, comp_t, table_t, out_t, want_status: bool):
    """``entry`` (a ``rocco_hip_*_inflate``) over CUDA tensors: (int32 status per block or None, int64 produced per block or None, the
    report).  The call returns when the kernels have run."""
    import torch

    for t, dtype in ((comp_t, torch.uint8), (table_t, torch.int64), (out_t, torch.uint8)):
        if not _dp._is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.device != out_t.device:
            raise TypeError(f"{who}: contiguous CUDA tensors on one device are required (uint8, int64, uint8)")
    if table_t.numel() % columns:
        raise ValueError(f"{who}: the block table has {columns} columns")
    n_blocks = table_t.numel() // columns
    status = torch.empty(n_blocks, dtype=torch.int32, device=out_t.device) if want_status else None
    produced = torch.empty(n_blocks, dtype=torch.int64, device=out_t.device) if with_produced else None
    back = (ctypes.c_longlong * 4)()
    per_block = [status.data_ptr() if status is not None and n_blocks else None] + ([produced.data_ptr() if n_blocks else None] if with_produced else [])
    with torch.cuda.device(out_t.device):
        _native.check(getattr(_native.load(), entry)(
            _native.solver_for(out_t.device.index).handle, comp_t.data_ptr() or None, comp_t.numel(), table_t.data_ptr() or None, n_blocks,
            out_t.data_ptr() or None, out_t.numel(), *per_block, back, _dp._stream_ptr(out_t)), entry)
    return status, produced, _report(back)


def inflate_blocks_host(comp, table: np.ndarray, out: np.ndarray):
    """`rocco_hip_bgzf_inflate_host` (test support: the kernels' decode rules compiled for the host, on the calling thread):
    inflates the rows of ``table`` from ``comp`` (bytes or a uint8 array) into the uint8 array ``out``; returns (the int32
    status per block, the report ``block`` / ``status`` / ``produced``)."""
    status, _, report = _blocks_host("inflate_blocks_host", "rocco_hip_bgzf_inflate_host", BGZF_TABLE_COLUMNS, False, comp, table, out)
    return status, report


def inflate_blocks_device(comp_t, table_t, out_t, want_status: bool = False):
    """`rocco_hip_bgzf_inflate`: inflates the rows of the int64 CUDA tensor ``table_t`` ([n][5]) from the uint8 CUDA tensor
    ``comp_t`` into the uint8 CUDA tensor ``out_t``; returns (the int32 status per block as a CUDA tensor, or None, the report)."""
    status, _, report = _blocks_device("inflate_blocks_device", "rocco_hip_bgzf_inflate", BGZF_TABLE_COLUMNS, False, comp_t, table_t, out_t, want_status)
    return status, report


def zlib_inflate_blocks_host(comp, table: np.ndarray, out: np.ndarray):
    """`rocco_hip_zlib_inflate_host` (test support: the kernels' rules compiled for the host, on the calling thread); returns
    (int32 status per block, int64 produced per block, the report ``block`` / ``status`` / ``produced``)."""
    return _blocks_host("zlib_inflate_blocks_host", "rocco_hip_zlib_inflate_host", ZLIB_TABLE_COLUMNS, True, comp, table, out)


def zlib_inflate_blocks_device(comp_t, table_t, out_t):
    """`rocco_hip_zlib_inflate`: inflates the rows of the int64 CUDA tensor ``table_t`` ([n][5]) from the uint8 CUDA tensor
    ``comp_t`` into the uint8 CUDA tensor ``out_t``; returns (int32 status, int64 produced per block as CUDA tensors, the report)."""
    return _blocks_device("zlib_inflate_blocks_device", "rocco_hip_zlib_inflate", ZLIB_TABLE_COLUMNS, True, comp_t, table_t, out_t, True)


def refuse_large_blocks(blocks, where) -> None:
    """ValueError for the first `_bgzf_blocks` row whose ISIZE exceeds what the device inflate holds; ``where(index, block)``
    words its place (asked only then: a file has tens of thousands of blocks)."""
    for index, block in enumerate(blocks):
        if block[4] > BGZF_MAX_ISIZE:
            raise ValueError(f"{where(index, block)}: length mismatch (ISIZE says {block[4]}, a BGZF block "
                             f"holds at most {BGZF_MAX_ISIZE} bytes; inflate=\"host\" reads a file that breaks this rule)")


# --------------------------------------------------------------------------------------------
# staging: the compressed buffer as coalesced spans, the one upload
# --------------------------------------------------------------------------------------------

class SpanList:
    """The compressed buffer of one upload: ``spans``, the runs [source bytes, first byte, size] that are copied one behind the
    other, and ``n_comp``, their bytes in all."""

    def __init__(self):
        self.spans, self.n_comp = [], 0

    def add(self, raw, lo: int, hi: int, max_gap: int = 0) -> int:
        """Appends ``raw[lo:hi]`` and returns its place in the compressed buffer.  It rides in the span before where that is
        of the same source (the same object) and ends at most ``max_gap`` bytes in front of ``lo``; the bytes between ride
        along (64 takes the trailer and the header between neighbouring BGZF blocks, 0 only what is exactly adjacent)."""
        last = self.spans[-1] if self.spans else None
        gap = lo - (last[1] + last[2]) if last is not None and last[0] is raw else -1
        if 0 <= gap <= max_gap:
            last[2] += gap + hi - lo
            self.n_comp += gap
        else:
            self.spans.append([raw, lo, hi - lo])
        at = self.n_comp
        self.n_comp += hi - lo
        return at


def upload_blocks(table: np.ndarray, spans, n_comp: int, dev):
    """The int64 block table in front of the ``n_comp`` bytes of ``spans`` ((source, first byte, size) each) in one pinned
    buffer, one non-blocking copy to ``dev``: (the table, the compressed bytes) as views of the uploaded tensor.  The copy is
    only queued: the pinned buffer stays bound to the second view, so keep that until a call that waits for the stream (the
    inflate does) has returned."""
    import torch

    table = np.ascontiguousarray(table, dtype=np.int64)
    head = table.size * 8
    staged = _host_buffer(head + int(n_comp))
    staged[:head] = table.reshape(-1).view(np.uint8)
    at = head
    for raw, first, size in spans:
        staged[at: at + size] = np.frombuffer(raw[first: first + size], dtype=np.uint8)
        at += size
    up = torch.from_numpy(staged).to(dev, non_blocking=True)
    table_t, comp_t = up[:head].view(torch.int64), up[head:]
    comp_t.staged = staged
    return table_t, comp_t
