"""Read the ``.bai`` index of a BAM file on the host (note (32)): per reference the bins with their
chunks of virtual offsets, the pseudo-bin 37450 (the virtual offsets of the reference's first record and of the end of its
last; its mapped and unmapped counts) and the trailing count of records without a contig.  `rocco_amd.bam.read_alignment_spans`
reads a contig of a file from `contig_span`; `_get_bam_count_metadata` takes the read counts from `contig_stats`, as the
reference's ``ccounts_getMappedReadCount`` does (``hts_idx_get_stat``).

A virtual offset is ``(the file offset of a BGZF block) << 16 | (a byte offset inside its inflated data)``.

Not read: ``.csi`` indexes (a file that has only one takes the whole-file route, as a file without an index does), the linear
index (its length is checked, its entries are skipped: nothing here asks for less than a contig)."""
from __future__ import annotations

import collections
import os
import struct
from typing import List, Optional, Tuple

import numpy as np

BAI_MAGIC = b"BAI\x01"
PSEUDO_BIN = 37450  # htslib's META_BIN for the five-level binning scheme of a BAI
_CHUNK = np.dtype([("begin", "<u8"), ("end", "<u8")])


class BamIndex:
    """What `open_bam_index` keeps of a file: ``name``, ``size``, per reference ``bins`` ({bin: uint64 array [n][2] of chunk
    (begin, end)}, the pseudo-bin left out), ``pseudo`` ((v_begin, v_end, n_mapped, n_unmapped) or None), ``n_intv`` (the length
    of its linear index), and ``n_no_coor`` (None where the file ends before it)."""

    def __init__(self, name: str, size: int, bins: list, pseudo: list, n_intv: list, n_no_coor: Optional[int]):
        self.name, self.size, self.bins, self.pseudo, self.n_intv, self.n_no_coor = name, size, bins, pseudo, n_intv, n_no_coor

    @property
    def n_ref(self) -> int:
        return len(self.bins)


def _bad(name: str, what: str, at: int, why: str) -> ValueError:
    return ValueError(f"{name}: {what} at file offset {at}: {why}")


def _need(raw, name: str, what: str, at: int, n: int) -> None:
    if at < 0 or n < 0 or at + n > len(raw):
        raise _bad(name, what, at, f"{n} bytes from there leave the file ({len(raw)} bytes)")


def parse_bam_index(raw, name: str = "<bytes>") -> BamIndex:
    """The parsed index from its bytes.  ValueError naming the file, the structure and the file offset for a count or an
    offset that leaves the file, a pseudo-bin without two chunks and a chunk whose end lies before its begin."""
    raw = memoryview(raw).cast("B") if not isinstance(raw, memoryview) else raw
    _need(raw, name, "the header", 0, 8)
    if bytes(raw[0:4]) != BAI_MAGIC:
        raise _bad(name, "the header", 0, f"magic {bytes(raw[0:4])!r} where {BAI_MAGIC!r} belongs (not a .bai index)")
    (n_ref,) = struct.unpack_from("<i", raw, 4)
    if n_ref < 0:
        raise _bad(name, "the header", 4, f"n_ref is negative ({n_ref})")
    return BamIndex(name, len(raw), *parse_index_body(raw, name, 8, n_ref))


def parse_index_body(raw, name: str, at: int, n_ref: int):
    """The per-reference body that a ``.bai`` and a ``.tbi`` index share, from file offset ``at``: (per reference its bins, its
    pseudo-bin, the length of its linear index; the trailing count of records without a contig or None).  The errors of
    `parse_bam_index`."""
    bins_of, pseudo_of, n_intv_of = [], [], []
    for tid in range(n_ref):
        what = f"reference {tid}"
        _need(raw, name, f"n_bin of {what}", at, 4)
        (n_bin,) = struct.unpack_from("<i", raw, at)
        if n_bin < 0:
            raise _bad(name, f"n_bin of {what}", at, f"it is negative ({n_bin})")
        _need(raw, name, f"the bins of {what}", at + 4, 8 * n_bin)  # (a bin has at least its number and its chunk count)
        at += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            _need(raw, name, f"a bin of {what}", at, 8)
            bin_id, n_chunk = struct.unpack_from("<Ii", raw, at)
            if n_chunk < 0:
                raise _bad(name, f"bin {bin_id} of {what}", at, f"n_chunk is negative ({n_chunk})")
            _need(raw, name, f"the chunks of bin {bin_id} of {what}", at + 8, 16 * n_chunk)
            chunks = np.frombuffer(raw, dtype=_CHUNK, count=n_chunk, offset=at + 8)
            if bin_id == PSEUDO_BIN:
                if n_chunk != 2:
                    raise _bad(name, f"the pseudo-bin {PSEUDO_BIN} of {what}", at, f"it has {n_chunk} chunks where 2 belong")
                if int(chunks["end"][0]) < int(chunks["begin"][0]):
                    raise _bad(name, f"the pseudo-bin {PSEUDO_BIN} of {what}", at + 8,
                               f"its span ends at virtual offset {int(chunks['end'][0])}, before its begin {int(chunks['begin'][0])}")
                pseudo = (int(chunks["begin"][0]), int(chunks["end"][0]), int(chunks["begin"][1]), int(chunks["end"][1]))
            else:
                backwards = np.flatnonzero(chunks["end"] < chunks["begin"])
                if backwards.size:
                    k = int(backwards[0])
                    raise _bad(name, f"chunk {k} of bin {bin_id} of {what}", at + 8 + 16 * k,
                               f"it ends at virtual offset {int(chunks['end'][k])}, before its begin {int(chunks['begin'][k])}")
                pairs = np.stack([chunks["begin"], chunks["end"]], axis=1) if n_chunk else np.zeros((0, 2), dtype=np.uint64)
                bins[int(bin_id)] = np.concatenate([bins[int(bin_id)], pairs]) if int(bin_id) in bins else pairs
            at += 8 + 16 * n_chunk
        _need(raw, name, f"n_intv of {what}", at, 4)
        (n_intv,) = struct.unpack_from("<i", raw, at)
        if n_intv < 0:
            raise _bad(name, f"n_intv of {what}", at, f"it is negative ({n_intv})")
        _need(raw, name, f"the linear index of {what}", at + 4, 8 * n_intv)
        at += 4 + 8 * n_intv
        bins_of.append(bins)
        pseudo_of.append(pseudo)
        n_intv_of.append(int(n_intv))
    n_no_coor = None
    if at + 8 <= len(raw):
        (n_no_coor,) = struct.unpack_from("<Q", raw, at)
    return bins_of, pseudo_of, n_intv_of, None if n_no_coor is None else int(n_no_coor)


_BAM_INDEX_CACHE: "collections.OrderedDict" = collections.OrderedDict()
BAM_INDEX_CACHE_FILES = 1024


def clear_bam_index_cache() -> None:
    """Drops every parsed index."""
    _BAM_INDEX_CACHE.clear()


def bam_index_path(bam_path) -> Optional[str]:
    """Where htslib finds the BAI of ``bam_path``: ``<path>.bai``, then the path with its extension replaced by ``.bai``."""
    bam_path = os.fspath(bam_path)
    for candidate in (bam_path + ".bai", os.path.splitext(bam_path)[0] + ".bai"):
        if os.path.isfile(candidate):
            return candidate
    return None


def open_bam_index(bam_path) -> Optional[BamIndex]:
    """The parsed ``.bai`` index of a BAM file, found as htslib finds it (`bam_index_path`), from the cache keyed on (path,
    size, mtime) or read now; None where there is none.  A ``.csi`` index is not read: a file that has only one gives None
    and takes the whole-file route.  ValueError (`parse_bam_index`) for an index that does not parse."""
    path = bam_index_path(bam_path)
    if path is None:
        return None
    stat = os.stat(path)
    key = (os.path.abspath(path), int(stat.st_size), int(stat.st_mtime_ns))
    hit = _BAM_INDEX_CACHE.get(key)
    if hit is not None:
        _BAM_INDEX_CACHE.move_to_end(key)
        return hit
    with open(path, "rb") as handle:
        index = parse_bam_index(memoryview(handle.read()), path)
    _BAM_INDEX_CACHE[key] = index
    while len(_BAM_INDEX_CACHE) > BAM_INDEX_CACHE_FILES:
        _BAM_INDEX_CACHE.popitem(last=False)
    return index


def bins_span(index: BamIndex, tid: int) -> Optional[Tuple[int, int]]:
    """(the minimum begin, the maximum end) over the chunks of the reference's bins, or None where it has none."""
    chunks = [c for c in index.bins[tid].values() if c.shape[0]] if 0 <= tid < index.n_ref else []
    if not chunks:
        return None
    return int(min(c[:, 0].min() for c in chunks)), int(max(c[:, 1].max() for c in chunks))


def contig_span(index: BamIndex, tid: int) -> Optional[Tuple[int, int]]:
    """``(v_begin, v_end)``: the virtual offsets of the reference's first record and of the end of its last -- the
    pseudo-bin's first chunk or, where there is no pseudo-bin, the minimum begin and maximum end over the bins.  None for a
    reference without bins (or one the index does not have)."""
    if not 0 <= tid < index.n_ref:
        return None
    pseudo = index.pseudo[tid]
    return (pseudo[0], pseudo[1]) if pseudo is not None else bins_span(index, tid)


def contig_stats(index: BamIndex, tid: int) -> Optional[Tuple[int, int]]:
    """``(n_mapped, n_unmapped)`` of the reference from its pseudo-bin (htslib's ``hts_idx_get_stat``), or None."""
    if not 0 <= tid < index.n_ref or index.pseudo[tid] is None:
        return None
    return index.pseudo[tid][2], index.pseudo[tid][3]


def chunk_list(index: BamIndex, tid: int) -> List[Tuple[int, int]]:
    """Every (begin, end) chunk of the reference's bins, sorted (test support)."""
    out = [(int(b), int(e)) for c in index.bins[tid].values() for b, e in c]
    return sorted(out)
