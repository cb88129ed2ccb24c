"""Read the ``.tbi`` index of a BGZF-compressed, tab-separated file on the host (note (34)).

A ``.tbi`` file is BGZF itself; inflated it holds the header ``TBI\\1``, n_ref, format, col_seq, col_beg, col_end, meta, skip,
l_nm and the NUL-separated sequence names in index order, then per reference the same body a ``.bai`` index has (bins with
chunks of virtual offsets, the pseudo-bin 37450, a linear index) and the trailing count of lines without a contig:
`rocco_amd.bam_index.parse_index_body` reads it for both.  `rocco_amd.fragments` reads a contig of a fragments file from
`rocco_amd.bam_index.contig_span` of what `open_tabix_index` returns.

Read: the BED preset of tabix (``TBX_UCSC``, columns 1 / 2 / 3, no skipped lines), which is what ``tabix -p bed`` writes and
what the reference's fragments source expects.  Not read: ``.csi`` and ``.tbi.csi`` indexes, the other presets."""
from __future__ import annotations

import collections
import os
import struct
from typing import List, Optional

from .bam_index import BamIndex, _bad, _need, parse_index_body

TBI_MAGIC = b"TBI\x01"
TBX_UCSC = 0x10000  # htslib's format word of the BED preset: generic columns, 0-based half-open coordinates
_HEADER = 36        # magic, n_ref, format, col_seq, col_beg, col_end, meta, skip, l_nm


class TabixIndex(BamIndex):
    """A `BamIndex` (``bins``, ``pseudo``, ``n_intv``, ``n_no_coor``) with what a ``.tbi`` adds: ``names`` (in index order),
    ``tid_of`` ({name: reference id}) and ``meta`` (the byte that begins a line the index iterator skips)."""

    def __init__(self, name: str, size: int, names: List[str], meta: int, body):
        super().__init__(name, size, *body)
        self.names, self.meta = names, meta
        self.tid_of = {}
        for tid, contig in enumerate(names):
            self.tid_of.setdefault(contig, tid)


def parse_tabix_index(raw, name: str = "<bytes>") -> TabixIndex:
    """The parsed index from its INFLATED bytes.  ValueError naming the file and the field for another magic, a format other
    than the BED preset, a name table that leaves the file or does not hold n_ref names; the errors of
    `rocco_amd.bam_index.parse_bam_index` for the body (offsets count in the inflated bytes)."""
    raw = memoryview(raw).cast("B") if not isinstance(raw, memoryview) else raw
    _need(raw, name, "the header", 0, _HEADER)
    if bytes(raw[0:4]) != TBI_MAGIC:
        raise _bad(name, "the header", 0, f"magic {bytes(raw[0:4])!r} where {TBI_MAGIC!r} belongs (not a .tbi index)")
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    if n_ref < 0:
        raise _bad(name, "the header", 4, f"n_ref is negative ({n_ref})")
    for field, at, found, wanted in (("format", 8, fmt, TBX_UCSC), ("col_seq", 12, col_seq, 1), ("col_beg", 16, col_beg, 2),
                                     ("col_end", 20, col_end, 3), ("skip", 28, skip, 0)):
        if found != wanted:
            raise _bad(name, f"{field} of the header", at,
                       f"it is {found} where the BED preset has {wanted} (only an index built with the BED preset is read)")
    if l_nm < 0:
        raise _bad(name, "l_nm of the header", 32, f"it is negative ({l_nm})")
    _need(raw, name, "the sequence names", _HEADER, l_nm)
    table = bytes(raw[_HEADER: _HEADER + l_nm])
    if l_nm and table[-1] != 0:
        raise _bad(name, "the sequence names", _HEADER, "the last name is not NUL-terminated")
    names = [part.decode("utf-8", "surrogateescape") for part in table.split(b"\x00")[:-1]] if l_nm else []
    if len(names) != n_ref:
        raise _bad(name, "the sequence names", _HEADER, f"they hold {len(names)} names where n_ref says {n_ref}")
    return TabixIndex(name, len(raw), names, meta, parse_index_body(raw, name, _HEADER + l_nm, n_ref))


_TABIX_INDEX_CACHE: "collections.OrderedDict" = collections.OrderedDict()
TABIX_INDEX_CACHE_FILES = 1024


def clear_tabix_index_cache() -> None:
    """Drops every parsed index."""
    _TABIX_INDEX_CACHE.clear()


def tabix_index_path(path) -> Optional[str]:
    """Where htslib's ``tbx_index_load`` finds the ``.tbi`` of ``path``: ``<path>.tbi``."""
    candidate = os.fspath(path) + ".tbi"
    return candidate if os.path.isfile(candidate) else None


def open_tabix_index(path) -> Optional[TabixIndex]:
    """The parsed ``.tbi`` index of a file, from the cache keyed on (path, size, mtime) or read and inflated now
    (`rocco_amd.bam.inflate_bgzf`); None where there is none (a ``.csi`` index is not read).  ValueError
    (`parse_tabix_index`, `inflate_bgzf`) for an index that does not inflate or parse."""
    from .bam import inflate_bgzf

    found = tabix_index_path(path)
    if found is None:
        return None
    stat = os.stat(found)
    key = (os.path.abspath(found), int(stat.st_size), int(stat.st_mtime_ns))
    hit = _TABIX_INDEX_CACHE.get(key)
    if hit is not None:
        _TABIX_INDEX_CACHE.move_to_end(key)
        return hit
    index = parse_tabix_index(memoryview(bytes(inflate_bgzf(found))), found)
    _TABIX_INDEX_CACHE[key] = index
    while len(_TABIX_INDEX_CACHE) > TABIX_INDEX_CACHE_FILES:
        _TABIX_INDEX_CACHE.popitem(last=False)
    return index
