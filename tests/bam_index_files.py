"""An independent ``.bai`` writer (test support): htslib's binning scheme (``reg2bin``), chunks per bin, the linear index and
the pseudo-bins, computed from a BAM file's own record walk (tests/bam_expected.py), so that tests make indexed files whose
BGZF blocks are cut where they choose (``bgzf_compress(cuts=...)``) -- and lying indexes.

Pinned to htslib: for every file of tests/golden/bam_index.npz the spans and statistics computed here equal those of the
``.bai`` htslib wrote (tests/test_bam_index_host.py).  The bins are NOT htslib's byte for byte: htslib merges the chunks of
small bins into their parents when it finishes an index (``compress_binning``), this writer keeps every run of records of one
bin as one chunk.  Nothing here reads rocco_amd."""
import os
import struct

import numpy as np

import bam_expected as bx

PSEUDO_BIN = 37450
LINEAR_SHIFT = 14
_golden = None


def golden():
    """(arrays, meta) of tests/golden/bam_index.npz / .json, loaded once and left unchanged."""
    global _golden
    if _golden is None:
        import json

        here = os.path.join(bx.HERE, "golden")
        with open(os.path.join(here, "bam_index.json"), encoding="utf-8") as handle:
            meta = json.load(handle)
        _golden = (dict(np.load(os.path.join(here, "bam_index.npz"))), meta)
    return _golden


def golden_bam(key: str) -> bytes:
    """The BAM bytes of an indexed fixture: the new files are stored with the index, the eight older ones in bam_files.npz."""
    arrays, _ = golden()
    return arrays[f"bam_{key}"].tobytes() if f"bam_{key}" in arrays else bx.bam_bytes(key)


def golden_bai(key: str) -> bytes:
    return golden()[0][f"bai_{key}"].tobytes()


def write_indexed(tmp_dir, key: str, bai: bytes = None, suffix: str = ".bam.bai") -> str:
    """The fixture and its index (or ``bai``) as files; returns the BAM's path."""
    path = os.path.join(str(tmp_dir), key + ".bam")
    with open(path, "wb") as handle:
        handle.write(golden_bam(key))
    with open(path[:-4] + suffix, "wb") as handle:
        handle.write(golden_bai(key) if bai is None else bai)
    return path


def reg2bin(beg: int, end: int) -> int:
    """htslib's hts_reg2bin for min_shift 14, n_lvls 5 (the SAM specification, section 5.3)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def block_table(raw: bytes):
    """(file offset, inflated offset, ISIZE) of every BGZF block."""
    rows, at, inflated = [], 0, 0
    while at < len(raw):
        (xlen,) = struct.unpack_from("<H", raw, at + 10)
        extra, bsize = at + 12, None
        while extra < at + 12 + xlen:
            si1, si2, slen = raw[extra], raw[extra + 1], struct.unpack_from("<H", raw, extra + 2)[0]
            if si1 == 66 and si2 == 67:
                bsize = struct.unpack_from("<H", raw, extra + 4)[0] + 1
            extra += 4 + slen
        (isize,) = struct.unpack_from("<I", raw, at + bsize - 4)
        rows.append((at, inflated, isize))
        at, inflated = at + bsize, inflated + isize
    return rows


def voffset(table, file_size: int, p: int, at_block_end: bool = False) -> int:
    """The virtual offset of inflated offset ``p`` as htslib's bgzf_tell states it after reading up to ``p``: inside a block,
    that block; on a boundary, the block that FOLLOWS the one just consumed at offset 0 (the first of several that begin at
    ``p``; the file's size where none does).  ``at_block_end``: on a boundary, the block just consumed at offset ISIZE
    instead (what older writers leave in an index, and what readers must accept)."""
    starts = [row[1] for row in table]
    first = int(np.searchsorted(starts, p, side="left"))
    if first < len(table) and starts[first] == p:  # a boundary
        if at_block_end and first > 0 and table[first - 1][2] > 0:
            return table[first - 1][0] << 16 | table[first - 1][2]
        return table[first][0] << 16
    if first == len(table) and table and p == table[-1][1] + table[-1][2]:
        if at_block_end and table[-1][2] > 0:
            return table[-1][0] << 16 | table[-1][2]
        return file_size << 16
    row = table[first - 1]
    assert row[1] < p < row[1] + row[2], (p, row)
    return row[0] << 16 | (p - row[1])


def facts(raw: bytes, at_block_end: bool = False) -> dict:
    """What an index says about a file, from its own record walk: ``n_ref``, ``records`` (offsets, tid, pos, end, flag per
    record), per reference the ``span`` (v_begin, v_end) or None and the ``stats`` (mapped, unmapped), ``n_no_coor``, and
    ``voffsets`` (the virtual offset of every record start, and of the end of the last)."""
    data, _ = bx.inflate(raw)
    _, contigs, entry0 = bx.header(data)
    offsets, end, why, _ = bx.walk(data, entry0)
    assert why == 0 and end == len(data)
    stated, _ = bx.fields(data, offsets, len(contigs))
    table = block_table(raw)
    edges = np.concatenate([offsets, [len(data)]]).astype(np.int64)
    v = np.asarray([voffset(table, len(raw), int(p), at_block_end and 0 < k) for k, p in enumerate(edges)], dtype=np.uint64)
    tid = stated["tid"].astype(np.int64)
    spans, stats = [], []
    for t in range(len(contigs)):
        mine = np.flatnonzero(tid == t)
        if mine.size == 0:
            spans.append(None)
            stats.append(None)
            continue
        assert np.array_equal(mine, np.arange(mine[0], mine[-1] + 1)), "the file is not sorted"
        spans.append((int(v[mine[0]]), int(v[mine[-1] + 1])))
        unmapped = int(np.count_nonzero(stated["flag"][mine] & 4))
        stats.append((int(mine.size) - unmapped, unmapped))
    return {"n_ref": len(contigs), "contigs": contigs, "offsets": offsets, "fields": stated, "spans": spans, "stats": stats,
            "n_no_coor": int(np.count_nonzero(tid < 0)), "voffsets": v, "inflated": len(data), "blocks": table}


def build_index(raw: bytes, at_block_end: bool = False, pseudo: bool = True) -> list:
    """Per reference {"bins": {bin: [(begin, end)]}, "pseudo": (v_begin, v_end, mapped, unmapped) or None, "linear": [...]}."""
    f = facts(raw, at_block_end)
    v, tid, pos, end = f["voffsets"], f["fields"]["tid"].astype(np.int64), f["fields"]["pos"].astype(np.int64), f["fields"]["end"].astype(np.int64)
    refs = []
    for t in range(f["n_ref"]):
        bins, linear = {}, []
        mine = np.flatnonzero(tid == t)
        run_bin, run_begin, run_end = None, 0, 0
        for r in mine.tolist():
            b = reg2bin(int(pos[r]), int(end[r]))
            if b != run_bin:
                if run_bin is not None:
                    bins.setdefault(run_bin, []).append((run_begin, run_end))
                run_bin, run_begin = b, int(v[r])
            run_end = int(v[r + 1])
            lo, hi = int(pos[r]) >> LINEAR_SHIFT, (int(end[r]) - 1) >> LINEAR_SHIFT
            while len(linear) <= hi:
                linear.append(None)
            for w in range(lo, hi + 1):
                if linear[w] is None:
                    linear[w] = int(v[r])
        if run_bin is not None:
            bins.setdefault(run_bin, []).append((run_begin, run_end))
        last = 0
        for w in range(len(linear)):  # (htslib fills the windows no record begins in with the offset before)
            if linear[w] is None:
                linear[w] = last
            last = linear[w]
        span, stats = f["spans"][t], f["stats"][t]
        refs.append({"bins": bins, "linear": linear,
                     "pseudo": (span[0], span[1], stats[0], stats[1]) if (pseudo and span is not None) else None})
    return refs, f["n_no_coor"]


def bai_bytes(refs, n_no_coor=None) -> bytes:
    out = [b"BAI\x01", struct.pack("<i", len(refs))]
    for ref in refs:
        n_bin = len(ref["bins"]) + (1 if ref["pseudo"] is not None else 0)
        out.append(struct.pack("<i", n_bin))
        for b in sorted(ref["bins"]):
            chunks = ref["bins"][b]
            out.append(struct.pack("<Ii", b, len(chunks)))
            out += [struct.pack("<QQ", begin, end) for begin, end in chunks]
        if ref["pseudo"] is not None:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, *ref["pseudo"]))
        out.append(struct.pack("<i", len(ref["linear"])))
        out += [struct.pack("<Q", o) for o in ref["linear"]]
    if n_no_coor is not None:
        out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def index_bytes(raw: bytes, at_block_end: bool = False, pseudo: bool = True, no_coor: bool = True) -> bytes:
    refs, n_no_coor = build_index(raw, at_block_end, pseudo)
    return bai_bytes(refs, n_no_coor if no_coor else None)


def synthetic_bam(contigs, records, cuts=(), tail=0) -> bytes:
    """A BAM file of ``records`` -- [(tid, total bytes)] in file order, tid ascending -- over ``contigs``, plus ``tail``
    records without a contig; ``cuts``: where the BGZF blocks end, as inflated offsets counted from the FIRST RECORD."""
    head = bx.make_header(contigs)
    body, at = b"", {}
    for tid, total in records:
        at[tid] = at.get(tid, 0) + 1
        body += bx.make_record(total, tid=tid, pos=100 * at[tid], flag=16 if at[tid] % 3 == 0 else 0, name=b"q%d\0" % (at[tid] % 10))
    for k in range(tail):
        body += bx.make_record(40, tid=-1, pos=-1, flag=4, name=b"u\0")
    return bx.bgzf_compress(head + body, [len(head) + c for c in cuts])


def write_pair(tmp_dir, name: str, raw: bytes, bai: bytes = None, **kw) -> str:
    path = os.path.join(str(tmp_dir), name + ".bam")
    with open(path, "wb") as handle:
        handle.write(raw)
    with open(path + ".bai", "wb") as handle:
        handle.write(index_bytes(raw, **kw) if bai is None else bai)
    return path
