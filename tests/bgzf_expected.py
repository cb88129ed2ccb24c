"""The cases the BGZF inflate of csrc/bgzf_inflate.hip / csrc/inflate_core.h is held against (note
(29)), and what each of them must give.  Pure Python and NumPy: a BGZF writer over `zlib.compressobj`, a bit writer for
streams zlib's compressor never emits, three case lists (valid files, corrupt files one per acceptance rule, seeded
mutations), and the expected outcome of a block, which is the existing host path's: the bytes where
`zlib.decompress(span, wbits=-15)` succeeds with the stated length and CRC32, else which of the three checks refused it."""
import struct
import zlib

import numpy as np

import bam_expected as bx

ERR_STREAM, ERR_LENGTH, ERR_CRC, ERR_TABLE = 1, 2, 3, 4
LEADING_WORDS = {ERR_STREAM: "the deflate stream does not inflate (", ERR_LENGTH: "length mismatch (ISIZE says {isize}, ", ERR_CRC: "CRC32 mismatch"}
EOF_BLOCK = bx.EOF_BLOCK


# ---- the BGZF writer -----------------------------------------------------------------------------------------------------
def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flushes=(), flush_mode: int = zlib.Z_FULL_FLUSH) -> bytes:
    """`data` as one raw deflate stream; `flushes`: byte offsets behind which the compressor is flushed with `flush_mode`."""
    packer = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = [], 0
    for cut in [c for c in flushes if 0 < c < len(data)]:
        out.append(packer.compress(data[at:cut]) + packer.flush(flush_mode))
        at = cut
    return b"".join(out) + packer.compress(data[at:]) + packer.flush()


def block(cdata: bytes, crc: int, isize: int, extra_first: bytes = b"", extra_last: bytes = b"") -> bytes:
    """One BGZF block around the deflate data `cdata` with the trailer as given; whole extra subfields before and behind BC."""
    xlen = len(extra_first) + 6 + len(extra_last)
    bsize = 12 + xlen + len(cdata) + 8
    assert bsize <= 0x10000, bsize
    return (struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra_first + b"BC" + struct.pack("<HH", 2, bsize - 1) + extra_last +
            cdata + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def packed(data: bytes, **how) -> bytes:
    """One sound BGZF block holding `data`, compressed as `deflate(data, **how)` does."""
    return block(deflate(data, **how), zlib.crc32(data), len(data))


def around(cdata: bytes, data: bytes) -> bytes:
    """One BGZF block whose deflate data is `cdata` and whose trailer states `data`."""
    return block(cdata, zlib.crc32(data), len(data))


# ---- the bit writer (RFC 1951: values go in from bit 0, Huffman codes most significant bit first) -----------------------------
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CODE_LENGTH_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lengths):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (0: no code)."""
    code, out = 0, {}
    for length in range(1, 16):
        for symbol, have in enumerate(lengths):
            if have == length:
                out[symbol] = (code, length)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


class Bits:
    def __init__(self):
        self.bits = []

    def value(self, v: int, n: int):
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, pair):
        code, n = pair
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def bytes(self) -> bytes:
        padded = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b << k for k, b in enumerate(padded[at: at + 8])) for at in range(0, len(padded), 8))

    # symbols of a block under the codes `lit` and `dist`
    def literal(self, byte: int, lit=FIXED_LIT):
        return self.code(lit[byte])

    def match(self, length: int, distance: int, lit=FIXED_LIT, dist=FIXED_DIST):
        ls = max(k for k in range(29) if LENGTH_BASE[k] <= length and (k < 28 or length == 258))
        ds = max(k for k in range(30) if DIST_BASE[k] <= distance)
        self.code(lit[257 + ls]).value(length - LENGTH_BASE[ls], LENGTH_EXTRA[ls])
        return self.code(dist[ds]).value(distance - DIST_BASE[ds], DIST_EXTRA[ds])

    def end(self, lit=FIXED_LIT):
        return self.code(lit[256])

    def header(self, final: int, kind: int):
        return self.value(final, 1).value(kind, 2)

    def dynamic(self, final: int, lit_lengths, dist_lengths, ops=None, hlit=None, hdist=None):
        """A dynamic block's header.  The code-length code is a complete one over all 19 symbols (0 .. 12 in 4 bits, 13 .. 18
        in 5); `ops`: the (symbol, extra value) sequence that states the lengths -- every length on its own where None."""
        cl = canonical(CL_LENGTHS)
        self.header(final, 2).value((len(lit_lengths) if hlit is None else hlit) - 257, 5)
        self.value((len(dist_lengths) if hdist is None else hdist) - 1, 5).value(19 - 4, 4)
        for symbol in CODE_LENGTH_ORDER:
            self.value(CL_LENGTHS[symbol], 3)
        for symbol, extra in (ops if ops is not None else [(v, 0) for v in list(lit_lengths) + list(dist_lengths)]):
            self.code(cl[symbol]).value(extra, {16: 2, 17: 3, 18: 7}.get(symbol, 0))
        return self


CL_LENGTHS = [4] * 13 + [5] * 6


def lengths(n: int, **given) -> list:
    out = [0] * n
    for symbol, length in given.items():
        out[int(symbol[1:])] = length
    return out


# ---- contents ------------------------------------------------------------------------------------------------------------
def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


_text = {}


def text_bytes(n: int, seed: int) -> bytes:
    """Text-like bytes: words of a small vocabulary, so a dynamic header states its lengths with the repeat codes 16, 17, 18."""
    if seed not in _text:
        rng = np.random.default_rng(seed)
        words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(300)]
        picks = (rng.integers(0, 300, size=20000) * rng.random(20000)).astype(np.int64)
        _text[seed] = b"".join(words[k] + (b"\n" if k % 10 == 0 else b" ") for k in picks)
        assert len(_text[seed]) >= 65536
    return _text[seed][:n]


_records = []


def record_bytes(n: int) -> bytes:
    """A real record stream: the inflated bytes of the `mixed` fixture, repeated to n bytes."""
    if not _records:
        _records.append(bx.inflate(bx.bam_bytes("mixed"))[0])
    data = _records[0]
    return (data * (n // len(data) + 1))[:n]


# ---- hand-assembled streams ------------------------------------------------------------------------------------------------
def hand_streams():
    """[(label, deflate data, the bytes it inflates to)]: fixed-Huffman streams zlib's compressor does not emit, and dynamic
    blocks at the allowed edge of the code-set rules."""
    out = []
    far = random_bytes(32768, 5)
    bits = Bits().header(1, 1)
    for byte in far:
        bits.literal(byte)
    out.append(("length 258 at distance 32768", bits.match(258, 32768).end().bytes(), far + far[:258]))
    for distance in (1, 2):
        for length in (3, 258):
            bits = Bits().header(1, 1).literal(120).literal(121).match(length, distance).literal(122).end()
            out.append((f"length {length} at distance {distance}", bits.bytes(), b"xy" + bytes((b"xy" * 200)[2 - distance + k % distance] for k in range(length)) + b"z"))
    # a complete literal/length code {97: 1 bit, 256: 2, 257: 2} and a distance set of ONE code of length 1, used
    lit, one = lengths(258, s97=1, s256=2, s257=2), [1]
    bits = Bits().dynamic(1, lit, one).literal(97, canonical(lit)).match(3, 1, canonical(lit), canonical(one)).end(canonical(lit))
    out.append(("a distance set of one code, used", bits.bytes(), b"aaaa"))
    # a literal/length set of one code of length 1 (256 alone) and no distance code at all
    lit = lengths(257, s256=1)
    out.append(("a literal/length set of one code, an empty distance set", Bits().dynamic(1, lit, [0]).end(canonical(lit)).bytes(), b""))
    # the lengths stated with 16, 17 and 18: 97 zeros, `a` and `b` in 2 bits, 157 zeros, 256 and 257 in 2 bits, and a 16 that
    # repeats the 2 of symbol 257 over the first three distance codes
    lit, dist = lengths(258, s97=2, s98=2, s256=2, s257=2), [2, 2, 2, 2]
    ops = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (17, 10 - 3), (17, 9 - 3), (2, 0), (2, 0), (16, 0), (2, 0)]
    bits = Bits().dynamic(1, lit, dist, ops=ops)
    bits.literal(97, canonical(lit)).literal(98, canonical(lit)).match(3, 2, canonical(lit), canonical(dist)).end(canonical(lit))
    out.append(("repeat codes 16, 17, 18 across the literal/distance boundary", bits.bytes(), b"ababa"))
    return out


# ---- the valid files -------------------------------------------------------------------------------------------------------
_valid = None


def valid_files():
    """[(label, the bytes of a BGZF file)], built once."""
    global _valid
    if _valid is not None:
        return _valid
    files = []
    for n in (0, 1, 2, 63, 64, 65, 257, 258, 259, 65280):
        files.append((f"{n} random bytes", packed(random_bytes(n, n)) + EOF_BLOCK))
    files.append(("65536 bytes of one value", packed(b"\x07" * 65536) + EOF_BLOCK))
    contents = {"random": random_bytes(65280, 1), "text": text_bytes(65280, 2), "records": record_bytes(65280)}
    for level in (0, 1, 6, 9):
        for kind, data in contents.items():
            files.append((f"level {level}, {kind}", packed(data, level=level) + EOF_BLOCK))
    for name in ("Z_FIXED", "Z_HUFFMAN_ONLY", "Z_RLE"):
        for kind in ("text", "records"):
            files.append((f"{name}, {kind}", packed(contents[kind][:30000], strategy=getattr(zlib, name)) + EOF_BLOCK))
    files.append(("Z_RLE, 65536 zeros", packed(bytes(65536), strategy=zlib.Z_RLE) + EOF_BLOCK))
    for name in ("Z_FULL_FLUSH", "Z_SYNC_FLUSH"):
        for kind in ("text", "records"):
            files.append((f"{name} between deflate blocks, {kind}",
                          packed(contents[kind][:40000], flushes=(1, 1000, 1001, 20000, 39999), flush_mode=getattr(zlib, name)) + EOF_BLOCK))
    for label, cdata, data in hand_streams():
        files.append((f"hand-assembled: {label}", around(cdata, data) + EOF_BLOCK))
    small = [packed(text_bytes(100 + 7 * (k % 29), 100 + k % 13), level=(1, 6, 9)[k % 3]) if k % 3 else packed(record_bytes(150 + k % 200)[k % 50:])
             for k in range(600)]
    for count in (1, 2, 64, 65, 600):
        files.append((f"{count} blocks, end-of-file marker", b"".join(small[:count]) + EOF_BLOCK))
        files.append((f"{count} blocks, no end-of-file marker", b"".join(small[:count])))
        files.append((f"{count} blocks, end-of-file marker in the middle", b"".join(small[: (count + 1) // 2]) + EOF_BLOCK + b"".join(small[(count + 1) // 2: count])))
    data = contents["text"][:5000]
    files.append(("three bytes of garbage behind the final deflate block", around(deflate(data) + b"\xde\xad\x3f", data) + EOF_BLOCK))
    sub = lambda tag, body: tag + struct.pack("<H", len(body)) + body
    files.append(("several extra subfields", block(deflate(data), zlib.crc32(data), len(data), sub(b"XY", b"hello") + sub(b"AB", b""), sub(b"ZZ", b"\0" * 9)) +
                  block(deflate(data[:77]), zlib.crc32(data[:77]), 77, b"", sub(b"BD", b"12")) + EOF_BLOCK))
    _valid = files
    return files


# ---- the corrupt files: one per acceptance rule ------------------------------------------------------------------------------
_corrupt = None


def corrupt_blocks():
    """[(label, one BGZF block that must be refused, the check that refuses it)]."""
    data = text_bytes(3000, 9)
    good = deflate(data)
    out = []
    stream = lambda label, cdata, says=b"abc": out.append((label, around(cdata, says), ERR_STREAM))
    stream("block type 3", Bits().header(1, 3).bytes())
    stream("LEN / NLEN mismatch", Bits().header(1, 0).align().value(3, 16).value(~3 & 0xFFFF ^ 0x100, 16).bytes() + b"abc")
    lit, dist = lengths(258, s97=1, s256=2, s257=2), [1, 1]
    stream("HLIT 287", Bits().dynamic(1, lit, dist, hlit=287).bytes() + bytes(40))
    stream("HDIST 31", Bits().dynamic(1, lit, dist, hdist=31).bytes() + bytes(40))
    stream("a repeat past the end of the lengths", Bits().dynamic(1, lengths(257), [0], ops=[(18, 127), (18, 127)]).bytes() + bytes(8))
    stream("a leading 16", Bits().dynamic(1, lengths(257), [0], ops=[(16, 0)] + [(0, 0)] * 255).bytes() + bytes(8))
    stream("no code for 256", Bits().dynamic(1, lengths(258, s97=1, s98=1), dist).bytes() + bytes(8))
    stream("an over-subscribed literal/length set", Bits().dynamic(1, lengths(258, s97=1, s98=1, s256=1), dist).bytes() + bytes(8))
    stream("an incomplete literal/length set", Bits().dynamic(1, lengths(258, s97=2, s256=2), dist).bytes() + bytes(8))
    stream("an over-subscribed distance set", Bits().dynamic(1, lit, [1, 1, 1]).bytes() + bytes(8))
    stream("an incomplete distance set", Bits().dynamic(1, lit, [2, 2]).bytes() + bytes(8))
    stream("an incomplete code-length code", Bits().header(1, 2).value(0, 5).value(0, 5).value(0, 4).value(1, 3).value(0, 9).bytes() + bytes(8))
    one = [1]
    missing = Bits().dynamic(1, lit, one).literal(97, canonical(lit)).code(canonical(lit)[257]).value(1, 1)  # the distance code `1`: not in the set
    stream("the missing code of a one-code distance set", missing.bytes() + bytes(8), b"aaaa")
    only = lengths(257, s256=1)
    stream("the missing code of a one-code literal/length set", Bits().dynamic(1, only, [0]).value(1, 1).bytes() + bytes(8), b"")
    empty = Bits().dynamic(1, lit, [0]).literal(97, canonical(lit)).code(canonical(lit)[257]).value(0, 1)
    stream("a length symbol under an empty distance set", empty.bytes() + bytes(8), b"aaaa")
    stream("literal/length symbol 286 of the fixed code", Bits().header(1, 1).literal(97).code(FIXED_LIT[286]).bytes() + bytes(8))
    stream("distance symbol 30 of the fixed code", Bits().header(1, 1).literal(97).code(FIXED_LIT[257]).code(FIXED_DIST[30]).bytes() + bytes(8))
    stream("a distance too far back at output position 0", Bits().header(1, 1).match(3, 1).end().bytes(), b"aaa")
    five = Bits().header(1, 1)
    for byte in b"hello":
        five.literal(byte)
    stream("a distance too far back at output position 5", five.match(3, 6).end().bytes(), b"hellohel")
    stream("the span cut 1 byte short", good[:-1], data)
    stream("the span cut 3 bytes short", good[:-3], data)
    stream("an empty span", b"", b"")
    stream("a stored block cut short", Bits().header(1, 0).align().value(10, 16).value(~10 & 0xFFFF, 16).bytes() + b"abcde", b"abcdeabcde")
    too_long_then_bad = deflate(data, flushes=(2000,))[:-3]  # inflates past a short ISIZE and breaks after: zlib's error stands
    out.append(("too long for ISIZE and cut short behind", block(too_long_then_bad, zlib.crc32(data[:100]), 100), ERR_STREAM))
    out.append(("ISIZE one too small", block(good, zlib.crc32(data), len(data) - 1), ERR_LENGTH))
    out.append(("ISIZE one too large", block(good, zlib.crc32(data), len(data) + 1), ERR_LENGTH))
    out.append(("ISIZE 0 for a stream that inflates to 3000 bytes", block(good, zlib.crc32(data), 0), ERR_LENGTH))
    out.append(("ISIZE too small under a match that straddles it", block(deflate(b"ab" * 1500), zlib.crc32(b"ab" * 1500), 100), ERR_LENGTH))
    out.append(("one flipped CRC32 bit", block(good, zlib.crc32(data) ^ 0x00400000, len(data)), ERR_CRC))
    flipped = bytearray(data)
    flipped[1234] ^= 0x10
    out.append(("one flipped payload bit under a stored block", block(deflate(bytes(flipped), level=0), zlib.crc32(data), len(data)), ERR_CRC))
    return out


def corrupt_files():
    """[(label, the bytes of a BGZF file, the index of the block that must be refused, the check that refuses it)], built once:
    every corrupt block between two sound ones, then the bad block first, in the middle and last in files of 3 and 65."""
    global _corrupt
    if _corrupt is not None:
        return _corrupt
    sound = [packed(text_bytes(200 + 11 * k, 40 + k), level=(1, 6, 9)[k % 3]) for k in range(65)]
    blocks = corrupt_blocks()
    files = [(label, sound[0] + bad + sound[1] + EOF_BLOCK, 1, code) for label, bad, code in blocks]
    by_code = {code: bad for _, bad, code in blocks}
    for count in (3, 65):
        for where, at in (("first", 0), ("in the middle", count // 2), ("last", count - 1)):
            for code, name in ((ERR_STREAM, "stream"), (ERR_LENGTH, "length"), (ERR_CRC, "CRC32")):
                body = sound[:at] + [by_code[code]] + sound[at + 1: count]
                files.append((f"a {name} error {where} of {count} blocks", b"".join(body) + (EOF_BLOCK if code != ERR_CRC else b""), at, code))
    two = sound[:2] + [by_code[ERR_CRC], by_code[ERR_STREAM]] + sound[4:6]
    files.append(("a CRC32 error in front of a stream error: the first in file order", b"".join(two), 2, ERR_CRC))
    _corrupt = files
    return files


# ---- the mutation set --------------------------------------------------------------------------------------------------------
MUTATIONS = 2000
_mutations = None


def mutation_file():
    """One file of MUTATIONS blocks (seeded): each a sound block of at most 2 KiB of payload with one byte of its deflate data
    replaced or one bit of it flipped, under the sound block's trailer."""
    global _mutations
    if _mutations is not None:
        return _mutations
    rng = np.random.default_rng(2024)
    bases = []
    for k in range(24):
        n = int(rng.integers(1, 2049))
        data = (text_bytes, random_bytes, lambda n, seed: record_bytes(n + seed)[seed:])[k % 3](n, 300 + k)
        how = [dict(level=1), dict(level=6), dict(level=9), dict(level=0), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_RLE),
               dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(level=6, flushes=(n // 2,), flush_mode=zlib.Z_SYNC_FLUSH)][k % 8]
        bases.append((deflate(data, **how), data))
    for label, cdata, data in hand_streams()[1:]:
        bases.append((cdata, data))
    out = []
    for _ in range(MUTATIONS):
        cdata, data = bases[int(rng.integers(0, len(bases)))]
        changed = bytearray(cdata)
        at = int(rng.integers(0, len(changed)))
        if rng.random() < 0.5:
            changed[at] ^= 1 << int(rng.integers(0, 8))
        else:
            changed[at] = int(rng.integers(0, 256))
        out.append(around(bytes(changed), data))
    _mutations = b"".join(out)
    return _mutations


# ---- what a file must give -----------------------------------------------------------------------------------------------------
def blocks_of(raw: bytes):
    """`rocco_amd.bam._bgzf_blocks`: (file offset, first byte of the deflate data, one past its last, CRC32, ISIZE) per block."""
    from rocco_amd import bam

    return bam._bgzf_blocks(memoryview(raw), "<bytes>")


def outcomes(raw: bytes):
    """Per block (0, its bytes) or (the check that refuses it, None): the host path's three checks in the host path's order."""
    out = []
    for _, lo, hi, crc, isize in blocks_of(raw):
        try:
            data = zlib.decompress(raw[lo:hi], wbits=-15)
        except zlib.error:
            out.append((ERR_STREAM, None))
            continue
        out.append((ERR_LENGTH, None) if len(data) != isize else ((ERR_CRC, None) if zlib.crc32(data) != crc else (0, data)))
    return out


def table_of(raw: bytes) -> np.ndarray:
    """The block table of include/rocco_hip.h for the whole file: int64 [n][5], the offsets a prefix sum of ISIZE."""
    rows = blocks_of(raw)
    table = np.zeros((len(rows), 5), dtype=np.int64)
    at = 0
    for k, (_, lo, hi, crc, isize) in enumerate(rows):
        table[k] = (lo, hi, isize, crc, at)
        at += isize
    return table


def error_pattern(raw: bytes, index: int, code: int) -> str:
    """The regular expression a ValueError for block `index` must match: the host's prefix and leading words."""
    import re

    at, _, _, _, isize = blocks_of(raw)[index]
    return re.escape(f"<bytes>: BGZF block {index} at file offset {at}: " + LEADING_WORDS[code].format(isize=isize))


GUARD, GUARD_BYTE = 48, 0xA5


def guarded_table(raw: bytes):
    """(`table_of(raw)` with GUARD bytes in front of, between and behind the blocks' ranges; the size of that output buffer)."""
    table = table_of(raw)
    table[:, 4] += GUARD * (1 + np.arange(table.shape[0]))
    return table, int(table[:, 2].sum()) + GUARD * (table.shape[0] + 1)


def verify(raw: bytes, table: np.ndarray, status: np.ndarray, out: np.ndarray, label: str = "") -> int:
    """`status` and `out` (filled with GUARD_BYTE before the call) against `outcomes(raw)`: every block's status code, the bytes
    of every accepted block, and not one byte changed outside the blocks' ranges.  Returns the index of the first refused
    block or -1."""
    want = outcomes(raw)
    assert len(want) == table.shape[0] == status.shape[0], label
    inside = np.zeros(out.shape[0], dtype=bool)
    first = -1
    for k, (code, data) in enumerate(want):
        at, isize = int(table[k, 4]), int(table[k, 2])
        inside[at: at + isize] = True
        assert int(status[k]) & 0xFF == code and (code == ERR_STREAM) == (int(status[k]) >> 8 != 0), (label, k, int(status[k]), code)
        if code == 0:
            assert out[at: at + isize].tobytes() == data, (label, k)
        elif first < 0:
            first = k
    assert np.all(out[~inside] == GUARD_BYTE), (label, "a byte outside the blocks' ranges was written")
    return first
