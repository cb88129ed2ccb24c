"""A NumPy / pure-Python statement of what rocco_amd/bam.py and csrc/bam_records.hip compute:
BGZF inflate, the BAM header, the sequential record walk, the record fields and their checks, and the plausibility predicate
of the guess -- the same lines as csrc/bam_record.h, which is where the predicate is written for the device.  Also the two
builders the tests and tests/golden/make_golden_bam_files.py share: BGZF blocks of chosen sizes and synthetic records."""
import json
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GUESS_DEPTH = 3
DEFAULT_SEGMENT_BYTES = 16384
RUNOFF_BYTES = 65536  # a chain may end this far past the stream's end, no further (csrc/bam_record.h says why)
FIXED = 36
FIELDS = [("tid", np.int32), ("pos", np.int32), ("end", np.int32), ("isize", np.int32), ("flag", np.uint16), ("mapq", np.uint8),
          ("mate_same", np.uint8), ("qlen", np.int32)]
ERR_BLOCK_SIZE, ERR_TRUNCATED, ERR_SIZES, ERR_READ_NAME, ERR_REF_ID, ERR_CIGAR_SEQ, ERR_POSITION, ERR_END, ERR_CG_TAG, ERR_ORDER, \
    ERR_OFFSET = range(1, 12)


# ---- fixtures ------------------------------------------------------------------------------------------------------------
_golden = None


def golden():
    """(arrays, meta) of tests/golden/bam_files.npz / .json, loaded once and left unchanged."""
    global _golden
    if _golden is None:
        arrays = np.load(os.path.join(HERE, "golden", "bam_files.npz"))
        with open(os.path.join(HERE, "golden", "bam_files.json"), encoding="utf-8") as handle:
            _golden = ({k: arrays[k] for k in arrays.files}, json.load(handle))
    return _golden


def bam_bytes(key) -> bytes:
    return golden()[0][f"bam_{key}"].tobytes()


def dump(key) -> dict:
    """htslib's own decoding of every record of fixture `key`, in file order."""
    return {name: golden()[0][f"d_{key}_{name}"] for name, _ in FIELDS}


def write_bam(tmp_dir, key) -> str:
    path = os.path.join(str(tmp_dir), key + ".bam")
    with open(path, "wb") as handle:
        handle.write(bam_bytes(key))
    return path


# ---- BGZF ----------------------------------------------------------------------------------------------------------------
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data: bytes, extra_first: bytes = b"", level: int = 6) -> bytes:
    """One BGZF block holding `data` (at most 65 280 bytes); `extra_first`: whole extra subfields placed in front of BC."""
    assert len(data) <= 0xFF00
    packer = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = packer.compress(data) + packer.flush()
    xlen = len(extra_first) + 6
    bsize = 12 + xlen + len(cdata) + 8
    assert bsize <= 0x10000
    return (struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra_first + b"BC" + struct.pack("<HH", 2, bsize - 1) + cdata +
            struct.pack("<II", zlib.crc32(data), len(data)))


def bgzf_compress(data: bytes, cuts=(), eof: bool = True, extra_first: bytes = b"") -> bytes:
    """`data` as BGZF blocks that end at the ascending byte offsets `cuts` (and at most 65 280 bytes each)."""
    edges = sorted({0, len(data), *[c for c in cuts if 0 < c < len(data)]})
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        for at in range(lo, hi, 0xFF00):
            out.append(bgzf_block(data[at: min(hi, at + 0xFF00)], extra_first))
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def inflate(raw: bytes):
    """(the inflated bytes, the inflated offset at which every block begins) of a BGZF file; asserts where it is malformed."""
    out, starts, at = [], [], 0
    while at < len(raw):
        assert raw[at: at + 3] == b"\x1f\x8b\x08" and raw[at + 3] & 4
        (xlen,) = struct.unpack_from("<H", raw, at + 10)
        sub, bsize = at + 12, None
        while sub < at + 12 + xlen:
            si1, si2, slen = raw[sub], raw[sub + 1], struct.unpack_from("<H", raw, sub + 2)[0]
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", raw, sub + 4)[0] + 1
            sub += 4 + slen
        assert bsize is not None and at + bsize <= len(raw)
        data = zlib.decompress(raw[at + 12 + xlen: at + bsize - 8], wbits=-15)
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        assert zlib.crc32(data) == crc and len(data) == isize
        starts.append(sum(len(d) for d in out))
        out.append(data)
        at += bsize
    return b"".join(out), starts


# ---- the header ----------------------------------------------------------------------------------------------------------
def header(data: bytes):
    """(text, [(name, length)], offset of the first record)."""
    assert data[:4] == b"BAM\x01"
    (l_text,) = struct.unpack_from("<i", data, 4)
    text = data[8: 8 + l_text].split(b"\0", 1)[0].decode()
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, at)
    at += 4
    contigs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, at)
        name = data[at + 4: at + 4 + l_name - 1].decode()
        (l_ref,) = struct.unpack_from("<i", data, at + 4 + l_name)
        contigs.append((name, l_ref))
        at += 8 + l_name
    return text, contigs, at


def make_header(contigs, text: str = "") -> bytes:
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs))
    for name, length in contigs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out


# ---- the sequential walk -------------------------------------------------------------------------------------------------
def i32(data, o):
    return struct.unpack_from("<i", data, o)[0]


def walk(data: bytes, entry0: int, n_bytes=None):
    """(record offsets, the offset behind the last complete record, why the walk stopped, where): the chain from entry0."""
    n_bytes = len(data) if n_bytes is None else n_bytes
    offsets, p = [], entry0
    while p != n_bytes:
        if p + 4 > n_bytes:
            return np.asarray(offsets, dtype=np.int64), p, ERR_TRUNCATED, p
        block_size = i32(data, p)
        if block_size < 32:
            return np.asarray(offsets, dtype=np.int64), p, ERR_BLOCK_SIZE, p
        if p + 4 + block_size > n_bytes:
            return np.asarray(offsets, dtype=np.int64), p, ERR_TRUNCATED, p
        offsets.append(p)
        p += 4 + block_size
    return np.asarray(offsets, dtype=np.int64), p, 0, -1


# ---- the plausibility predicate (csrc/bam_record.h: bam_plausible_header, bam_plausible_chain) -----------------------------
def plausible_header(data, o: int, n_ref: int) -> bool:
    block_size, ref, l_seq, next_ref = i32(data, o), i32(data, o + 4), i32(data, o + 20), i32(data, o + 24)
    l_read_name, n_cigar = data[o + 12], struct.unpack_from("<H", data, o + 16)[0]
    return (block_size >= 32 and -1 <= ref < n_ref and -1 <= next_ref < n_ref and l_read_name >= 1 and l_seq >= 0 and
            4 * n_cigar + l_read_name + (l_seq + 1) // 2 + l_seq <= block_size - 32)


def plausible_chain(data, o: int, n_ref: int, n_bytes=None, depth: int = GUESS_DEPTH) -> bool:
    n_bytes = len(data) if n_bytes is None else n_bytes
    if o < 0 or o + FIXED > n_bytes or not plausible_header(data, o, n_ref):
        return False
    p = o + 4 + i32(data, o)
    for _ in range(1, depth):
        if p + FIXED > n_bytes:
            return p - n_bytes < RUNOFF_BYTES
        if not plausible_header(data, p, n_ref):
            return False
        p += 4 + i32(data, p)
    return p - n_bytes < RUNOFF_BYTES


def candidate_mask(data: bytes, n_ref: int) -> np.ndarray:
    """Vectorised first test of every offset: where plausible_header can hold at all (the chain is then tested one by one)."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    n = a.size - FIXED + 1
    if n <= 0:
        return np.zeros(0, dtype=bool)

    def word(at):
        v = a[at: at + n] | (a[at + 1: at + 1 + n] << 8) | (a[at + 2: at + 2 + n] << 16) | (a[at + 3: at + 3 + n] << 24)
        return np.where(v >= 1 << 31, v - (1 << 32), v)

    block_size, ref, l_seq, next_ref = word(0), word(4), word(20), word(24)
    l_read_name, n_cigar = a[12: 12 + n], a[16: 16 + n] | (a[17: 17 + n] << 8)
    return ((block_size >= 32) & (ref >= -1) & (ref < n_ref) & (next_ref >= -1) & (next_ref < n_ref) & (l_read_name >= 1) & (l_seq >= 0) &
            (4 * n_cigar + l_read_name + (l_seq + 1) // 2 + l_seq <= block_size - 32))


def guesses(data: bytes, entry0: int, n_ref: int, segment_bytes: int) -> np.ndarray:
    """The guess of every segment as the device makes it (guess_mode 1): -1 is none."""
    S = segment_bytes
    n_segments = max((len(data) + S - 1) // S, 1)
    out = np.full(n_segments, -1, dtype=np.int64)
    seg0 = entry0 // S
    if seg0 < n_segments and entry0 < len(data):  # (a stream that ends with its header has no chain to enter)
        out[seg0] = entry0
    hits = np.flatnonzero(candidate_mask(data, n_ref))
    hits = hits[hits >= (seg0 + 1) * S]
    for o in hits:
        i = int(o) // S
        if out[i] < 0 and plausible_chain(data, int(o), n_ref):
            out[i] = int(o)
    return out


def true_entries(data: bytes, entry0: int, segment_bytes: int) -> np.ndarray:
    """The first true record start of every segment (-1: none), for a stream the walk follows to its end."""
    offsets, _, _, _ = walk(data, entry0)
    n_segments = max((len(data) + segment_bytes - 1) // segment_bytes, 1)
    out = np.full(n_segments, -1, dtype=np.int64)
    for o in offsets[::-1]:
        out[int(o) // segment_bytes] = int(o)
    return out


def wrong_guesses(data: bytes, entry0: int, n_ref: int, segment_bytes: int) -> int:
    return int(np.count_nonzero(guesses(data, entry0, n_ref, segment_bytes) != true_entries(data, entry0, segment_bytes)))


# ---- the record fields ---------------------------------------------------------------------------------------------------
def fields(data: bytes, offsets, n_ref: int):
    """({field: array}, first error (code, record) or (0, -1)) as rocco_hip_bam_record_fields states them."""
    out = {name: np.zeros(len(offsets), dtype=dtype) for name, dtype in FIELDS}
    errors = []
    key_before = None
    for r, p in enumerate(int(o) for o in offsets):
        block_size, tid, pos = i32(data, p), i32(data, p + 4), i32(data, p + 8)
        l_read_name, mapq = data[p + 12], data[p + 13]
        n_cigar, flag = struct.unpack_from("<HH", data, p + 16)
        l_seq, mtid, isize = i32(data, p + 20), i32(data, p + 24), i32(data, p + 32)
        found = []
        sizes_ok = l_seq >= 0 and 4 * n_cigar + l_read_name + (l_seq + 1) // 2 + l_seq <= block_size - 32
        if not sizes_ok:
            found.append(ERR_SIZES)
        if l_read_name < 1:
            found.append(ERR_READ_NAME)
        if not (-1 <= tid < n_ref and -1 <= mtid < n_ref):
            found.append(ERR_REF_ID)
        if tid >= 0 and pos < 0:
            found.append(ERR_POSITION)
        rlen = cigar_qlen = 0
        if sizes_ok:
            words = struct.unpack_from(f"<{n_cigar}I", data, p + FIXED + l_read_name)
            for word in words:
                op, length = word & 15, word >> 4
                rlen += length if op in (0, 2, 3, 7, 8) else 0
                cigar_qlen += length if op in (0, 1, 4, 7, 8) else 0
            if n_cigar > 0:
                if tid >= 0 and pos >= 0 and words[0] & 15 == 4 and words[0] >> 4 == l_seq:
                    found.append(ERR_CG_TAG)
                if not flag & 4 and l_seq > 0 and cigar_qlen != l_seq:
                    found.append(ERR_CIGAR_SEQ)
        if flag & 4:
            rlen = 0
        end = pos + (rlen or 1)
        if end >= 1 << 31:
            found.append(ERR_END)
        key = n_ref if tid < 0 else tid
        if key_before is not None and key_before > key:
            found.append(ERR_ORDER)
        key_before = key
        if found:
            errors.append((r, min(found)))
        values = dict(tid=tid, pos=pos, end=min(end, (1 << 31) - 1), isize=isize, flag=flag, mapq=mapq, mate_same=int(mtid == tid),
                      qlen=cigar_qlen if (l_seq <= 0 and n_cigar > 0) else l_seq)
        for name, _ in FIELDS:
            out[name][r] = values[name]
    first = (errors[0][1], errors[0][0]) if errors else (0, -1)
    return out, first


def contig_first(tid: np.ndarray, n_ref: int) -> np.ndarray:
    key = np.where(tid < 0, n_ref, tid)
    return np.concatenate([np.searchsorted(key, np.arange(n_ref + 1), side="left"), [tid.size]]).astype(np.int64)


# ---- synthetic records ---------------------------------------------------------------------------------------------------
def make_record(total: int, tid: int = 0, pos: int = 0, flag: int = 0, mapq: int = 30, name: bytes = b"r\0", cigar=(), l_seq: int = 0,
                mtid: int = -1, mpos: int = -1, isize: int = 0) -> bytes:
    """One well-formed record of exactly `total` bytes (the block_size word included); what the fields leave is a tag's bytes."""
    body = name + b"".join(struct.pack("<I", (length << 4) | op) for op, length in cigar) + b"\x11" * ((l_seq + 1) // 2) + b"\xff" * l_seq
    assert total >= FIXED + len(body)
    pad = total - FIXED - len(body)
    return (struct.pack("<iiiBBHHHiiii", total - 4, tid, pos, len(name), mapq, 4680, len(cigar), flag, l_seq, mtid, mpos, isize) + body +
            b"\x7f" * pad)
