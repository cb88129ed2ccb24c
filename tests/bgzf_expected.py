"""The cases the BGZF inflate of csrc/bgzf_inflate.hip / csrc/inflate_core.h is held against (note
(29)), and what each of them must give.  Pure Python and NumPy: a BGZF writer over `zlib.compressobj`, a bit writer for
streams zlib's compressor never emits, three case lists (valid files, corrupt files one per acceptance rule, seeded
mutations), a scanner that takes the census of what a stream makes a decoder do (`scan`, `census`) with the hand-assembled
streams that fill its holes (`census_streams`), and the expected outcome of a block, which is the existing host path's: the
bytes where `zlib.decompress(span, wbits=-15)` succeeds with the stated length and CRC32, else which of the three checks
refused it -- and for a refused stream zlib's own reason (`stream_reason`)."""
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

    def pair(self, length_symbol: int, length_extra: int, distance_symbol: int, distance_extra: int, lit=FIXED_LIT, dist=FIXED_DIST):
        """A match stated by its two symbols (0 .. 28, 0 .. 29) and the values of their extra bits: also 258 as 27 with 31."""
        assert 0 <= length_extra < 1 << LENGTH_EXTRA[length_symbol] and 0 <= distance_extra < 1 << DIST_EXTRA[distance_symbol]
        self.code(lit[257 + length_symbol]).value(length_extra, LENGTH_EXTRA[length_symbol])
        return self.code(dist[distance_symbol]).value(distance_extra, DIST_EXTRA[distance_symbol])

    def end(self, lit=FIXED_LIT):
        return self.code(lit[256])

    def header(self, final: int, kind: int):
        return self.value(final, 1).value(kind, 2)

    def stored(self, final: int, data: bytes):
        """A whole stored block: the header, the padding to a byte, LEN, NLEN and the bytes."""
        self.header(final, 0).align().value(len(data), 16).value(~len(data) & 0xFFFF, 16)
        for byte in data:
            self.value(byte, 8)
        return self

    def dynamic(self, final: int, lit_lengths, dist_lengths, ops=None, hlit=None, hdist=None, cl_lengths=None):
        """A dynamic block's header.  The code-length code is a complete one over all 19 symbols (0 .. 12 in 4 bits, 13 .. 18
        in 5), or the one with `cl_lengths`; `ops`: the (symbol, extra value) sequence that states the lengths -- every length
        on its own where None."""
        cl_lengths = CL_LENGTHS if cl_lengths is None else cl_lengths
        cl = canonical(cl_lengths)
        self.header(final, 2).value((len(lit_lengths) if hlit is None else hlit) - 257, 5)
        self.value((len(dist_lengths) if hdist is None else hdist) - 1, 5).value(19 - 4, 4)
        for symbol in CODE_LENGTH_ORDER:
            self.value(cl_lengths[symbol], 3)
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


# ---- hand-assembled streams for what no other valid case makes a decoder do (`census` below says what that is) -------------------
LANE_LENGTHS = (3, 63, 64, 65, 66, 67, 127, 128, 129, 257, 258)  # around one and two passes of 64 lanes, and the longest
LANE_DISTANCES = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259)
PAIR_ORDER = "ssffddsdfs"  # stored, fixed, dynamic: every ordered pair of block kinds once
STAGE_OFFSETS = (-8, -7, -6, -5, -4, -3, 0, 2)  # of a stored LEN word, from a staging window's edge
MAX_STORED = 0x10000 - 26 - 5  # the longest stored block `block` takes: 26 bytes of frame, 5 of stored header


def stage_bytes() -> int:
    """kStage of csrc/bgzf_inflate.hip: the bytes of a span that the kernel keeps in LDS in front of its bit reader."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rocco_amd", "csrc", "bgzf_inflate.hip")
    with open(path) as handle:
        (value,) = re.findall(r"constexpr int kStage = (\d+);", handle.read())
    return int(value)


def stage_edges():
    """[(span offset of a stored LEN word, LEN)] of the staging streams: STAGE_OFFSETS around the first and the second window
    edge with an empty stored block; 1 and 2 stored bytes where the bytes handed back reach below a window just staged."""
    at = []
    for edge in (stage_bytes(), 2 * stage_bytes()):
        at += [(edge + off, 0) for off in STAGE_OFFSETS] + [(edge - 6, 1), (edge - 5, 2)]
    return at


def _skewed_literals(n: int, seed: int, first: int) -> bytes:
    """n bytes of the 13 values first, first + 1, ...: each once, then value k with probability 2^-(k + 1) (its code has k + 1 bits)."""
    picks = np.minimum(np.random.default_rng(seed).geometric(0.5, size=n - 13) - 1, 12)
    return bytes(range(first, first + 13)) + bytes((first + picks).astype(np.uint8))


def _reach(distance: int):
    symbol = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return symbol, distance - DIST_BASE[symbol]


_more_streams = None


def census_streams():
    """[(label, deflate data, the bytes zlib inflates it to)], built once: the streams `census` needs beside `hand_streams()`."""
    global _more_streams
    if _more_streams is not None:
        return _more_streams
    out = []
    add = lambda label, cdata: out.append((label, cdata, zlib.decompress(cdata, wbits=-15)))
    ones = lambda n: (1 << n) - 1

    # long codes: literals in 1 .. 13 bits, 256 in 14, length symbols 27 and 28 (284, 285) in 15; distance symbols 0 .. 13 in
    # 1 .. 14 bits (0 .. 11 used), 28 and 29 in 15.  32 768 literals, then 258 as 284 + 31 at 32 768 (15 + 5 + 15 + 13 = 48 bits)
    lit = lengths(286, **{f"s{65 + k}": k + 1 for k in range(13)}, s256=14, s284=15, s285=15)
    dist = list(range(1, 15)) + [0] * 14 + [15, 15]
    lc, dc = canonical(lit), canonical(dist)
    bits = Bits().dynamic(1, lit, dist)
    for byte in _skewed_literals(32768, 71, 65):
        bits.literal(byte, lc)
    bits.pair(27, 31, 29, 8191, lc, dc).pair(28, 0, 29, 8191, lc, dc)  # 258 through 284 and through 285 at 32 768
    bits.pair(27, 30, 29, 0, lc, dc).pair(27, 0, 28, 8191, lc, dc)  # 257 at 24 577, 227 at 24 576
    for symbol in range(12):
        for extra in sorted({0, ones(DIST_EXTRA[symbol])}):
            bits.pair(27, (5 * symbol + extra) % 32, symbol, extra, lc, dc)
    add("long codes: 15 bits on 284 and 285 and on distances 28 and 29, a 48-bit symbol last", bits.pair(27, 31, 29, 8191, lc, dc).end(lc).bytes())

    # a second pair of sets: 15 bits on length symbols 20 and 26 (277, 283), distance symbols 26 .. 29 in 13, 14, 15, 15 bits
    lit = lengths(284, **{f"s{97 + k}": k + 1 for k in range(13)}, s256=14, s277=15, s283=15)
    dist = list(range(1, 13)) + [0] * 14 + [13, 14, 15, 15]
    lc, dc = canonical(lit), canonical(dist)
    bits = Bits().dynamic(1, lit, dist)
    for byte in _skewed_literals(16384, 73, 97):
        bits.literal(byte, lc)
    for symbol in list(range(12)) + [26, 27]:
        for extra in sorted({0, ones(DIST_EXTRA[symbol])}):
            bits.pair(20, 15 if extra else 0, symbol, extra, lc, dc).pair(26, 0 if extra else 31, symbol, extra, lc, dc)
    add("long codes: 15 bits on 277 and 283, distances 26 and 27 in 13 and 14 bits", bits.end(lc).bytes())

    # the code-length code with lengths 1 .. 7 (the only complete one: 1 2 3 4 5 6 7 7, on the symbols 0 1 2 3 5 16 17 18):
    # a 1, b 2, c 3, 256 .. 259 in 5 bits (a 5 and a 16 that repeats it three times), two distance codes of 1 bit
    lit, dist = lengths(260, s97=1, s98=2, s99=3, s256=5, s257=5, s258=5, s259=5), [1, 1]
    lc, dc = canonical(lit), canonical(dist)
    cl = lengths(19, s0=1, s1=2, s2=3, s3=4, s5=5, s16=6, s17=7, s18=7)
    ops = [(18, 97 - 11), (1, 0), (2, 0), (3, 0), (18, 138 - 11), (17, 10 - 3), (17, 7 - 3), (0, 0), (5, 0), (16, 0), (1, 0), (1, 0)]
    bits = Bits().dynamic(1, lit, dist, ops=ops, cl_lengths=cl).literal(97, lc).literal(98, lc).literal(99, lc)
    add("a code-length code with lengths 1 to 7", bits.match(3, 2, lc, dc).match(5, 1, lc, dc).end(lc).bytes())

    # the fixed code: every length symbol with its extra bits all zeros and all ones (258 as 284 + 31 among them)
    bits = Bits().header(1, 1)
    for byte in random_bytes(300, 72):
        bits.literal(byte)
    turn = 0
    for symbol in range(29):
        for extra in sorted({0, ones(LENGTH_EXTRA[symbol])}):
            bits.pair(symbol, extra, *_reach((1, 2, 3, 4, 7, 64, 100, 259, 300)[turn % 9]))
            turn += 1
    add("every length symbol at both ends of its extra bits", bits.end().bytes())

    # ... and every distance symbol, behind 32 768 literals
    bits = Bits().header(1, 1)
    for byte in random_bytes(32768, 74):
        bits.literal(byte)
    turn = 0
    for symbol in range(30):
        for extra in sorted({0, ones(DIST_EXTRA[symbol])}):
            bits.pair((0, 20, 28, 7)[turn % 4], 0, symbol, extra)
            turn += 1
    add("every distance symbol at both ends of its extra bits", bits.end().bytes())

    # the lane copies: per distance one stream; every length behind `distance` fresh literals (the whole source was written
    # since the last fence), then the same match again (its source is the first copy's bytes, or lies below them)
    for distance in LANE_DISTANCES:
        fresh = random_bytes(distance * len(LANE_LENGTHS), 500 + distance)
        bits = Bits().header(1, 1)
        for k, length in enumerate(LANE_LENGTHS):
            for byte in fresh[k * distance: (k + 1) * distance]:
                bits.literal(byte)
            bits.match(length, distance).match(length, distance)
        add(f"lane copies at distance {distance}: lengths {', '.join(map(str, LANE_LENGTHS))}, each twice", bits.end().bytes())

    # all nine ordered pairs of block kinds in one stream, the second stored block empty
    lit, one = lengths(258, s97=1, s256=2, s257=2), [1]
    lc, dc = canonical(lit), canonical(one)
    payloads = [b"hello", b"", b"xyz", b"pq"]
    bits = Bits()
    for k, kind in enumerate(PAIR_ORDER):
        final = int(k == len(PAIR_ORDER) - 1)
        if kind == "s":
            bits.stored(final, payloads.pop(0))
        elif kind == "f":
            bits.header(final, 1).literal(48 + k).literal(200 + k).match(4 + k, 2).end()
        else:
            bits.dynamic(final, lit, one).literal(97, lc).match(3, 1, lc, dc).end(lc)
    add("every ordered pair of block kinds: " + PAIR_ORDER, bits.bytes())

    stored = lambda n: Bits().header(1, 0).align().value(n, 16).value(~n & 0xFFFF, 16).bytes()
    add(f"the largest stored block: {MAX_STORED} bytes", stored(MAX_STORED) + random_bytes(MAX_STORED, 75))

    # the staging window: literals of a fixed block, a stored block of 0 .. 2 bytes whose LEN word begins at span offset
    # `at` (3 + 8 (at - 2) + 7 + 3 bits stand in front of it, padded to 8 at), a final fixed block
    for at, n in stage_edges():
        bits = Bits().header(0, 1)
        for byte in np.random.default_rng(at).integers(0, 144, size=at - 2).tolist():  # (8 bits each)
            bits.literal(byte)
        bits.end().stored(0, b"<>"[:n]).header(1, 1)
        for byte in b"behind the stored block":
            bits.literal(byte)
        add(f"a stored block of {n} bytes with LEN at span offset {at} (windows of {stage_bytes()} bytes)", bits.match(10, 5).end().bytes())
    _more_streams = out
    return out


# ---- the census: what a stream makes a decoder do ----------------------------------------------------------------------------------
def _decoder(code_lengths):
    """(table, mask): table[the stream's next bits & mask] = symbol << 4 | code length, 0 where no code of the set begins."""
    codes = canonical(code_lengths)
    width = max((n for _, n in codes.values()), default=1)
    table = np.zeros(1 << width, dtype=np.int64)
    for symbol, (code, n) in codes.items():
        table[int(format(code, f"0{n}b")[::-1], 2):: 1 << n] = symbol << 4 | n
    return table.tolist(), (1 << width) - 1


_FIXED_DECODERS = []


def scan(cdata: bytes, trace=None):
    """Walks a raw deflate stream that zlib accepts.  Returns (blocks, produced): per deflate block -- per code set -- a dict of
    `kind` (s, f, d), `lit_bits` and `dist_bits` (the code lengths of the decoded literal/length and distance symbols),
    `lengths` and `distances` ({(symbol, the value of its extra bits)}), `cl_bits` (the code-length code's lengths), `copies`
    ({(length, distance)}), `repeats` (those that follow the same match directly), `widest` (the bits of its longest length and
    distance symbol, extra bits included), `stored` ((the span offset of the LEN word, LEN) or None); and the bytes the stream
    inflates to.  `trace`: a list that receives (what, first bit, one past its last)
    of the fields a span can be cut in."""
    n = len(cdata)
    b = np.frombuffer(cdata + bytes(8), dtype=np.uint8).astype(np.int64)
    words = (b[: n + 4] | b[1: n + 5] << 8 | b[2: n + 6] << 16 | b[3: n + 7] << 24).tolist()  # 25 bits from any bit position
    p, produced, blocks = 0, 0, []
    note = (lambda what, s, e: trace.append((what, s, e))) if trace is not None else (lambda what, s, e: None)

    def take(k):
        nonlocal p
        v = (words[p >> 3] >> (p & 7)) & ((1 << k) - 1)
        p += k
        return v

    def symbol_of(table, mask):
        nonlocal p
        entry = table[(words[p >> 3] >> (p & 7)) & mask]
        if not entry:
            raise ValueError("scan: no code of the set begins here")
        p += entry & 15
        return entry >> 4

    final = 0
    while not final:
        final, kind = take(1), take(2)
        block = dict(kind="sfd"[kind], lit_bits=set(), dist_bits=set(), lengths=set(), distances=set(), cl_bits=set(), copies=set(),
                     repeats=set(), stored=None, widest=0)
        blocks.append(block)
        if kind == 0:
            p += -p % 8
            note("a stored LEN / NLEN", p, p + 32)
            size, check = take(16), take(16)
            if size != ~check & 0xFFFF:
                raise ValueError("scan: LEN / NLEN")
            block["stored"] = (p // 8 - 4, size)
            p += 8 * size
            produced += size
        else:
            if kind == 1:
                if not _FIXED_DECODERS:
                    _FIXED_DECODERS.extend([_decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _decoder([5] * 32)])
                lit_lengths, dist_lengths = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
                (lt, lm), (dt, dm) = _FIXED_DECODERS
            else:
                note("the HLIT / HDIST / HCLEN word", p, p + 14)
                nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
                note("the code-length code's lengths", p, p + 3 * ncode)
                cl = [0] * 19
                for k in range(ncode):
                    cl[CODE_LENGTH_ORDER[k]] = take(3)
                block["cl_bits"] = {v for v in cl if v}
                ct, cm = _decoder(cl)
                stated = []
                while len(stated) < nlen + ndist:
                    symbol = symbol_of(ct, cm)
                    if symbol < 16:
                        stated.append(symbol)
                    else:
                        width = {16: 2, 17: 3, 18: 7}[symbol]
                        note("a repeat code's extra bits", p, p + width)
                        stated += [stated[-1] if symbol == 16 else 0] * ({16: 3, 17: 3, 18: 11}[symbol] + take(width))
                if len(stated) != nlen + ndist:
                    raise ValueError("scan: a repeat past the lengths")
                lit_lengths, dist_lengths = stated[:nlen], stated[nlen:]
                (lt, lm), (dt, dm) = _decoder(lit_lengths), _decoder(dist_lengths)
            seen, dseen, before = [False] * 288, [False] * 32, None
            lengths_seen, distances_seen, copies, repeats = block["lengths"], block["distances"], block["copies"], block["repeats"]
            while True:
                entry = lt[(words[p >> 3] >> (p & 7)) & lm]
                if not entry:
                    raise ValueError("scan: no code of the set begins here")
                p += entry & 15
                symbol = entry >> 4
                seen[symbol] = True
                if symbol < 256:
                    produced += 1
                    before = None
                    continue
                if symbol == 256:
                    break
                first = p - (entry & 15)
                symbol -= 257
                width = LENGTH_EXTRA[symbol]
                extra = (words[p >> 3] >> (p & 7)) & ((1 << width) - 1)
                p += width
                at = p
                entry = dt[(words[p >> 3] >> (p & 7)) & dm]
                if not entry:
                    raise ValueError("scan: no code of the set begins here")
                p += entry & 15
                dsymbol = entry >> 4
                dseen[dsymbol] = True
                dwidth = DIST_EXTRA[dsymbol]
                dextra = (words[p >> 3] >> (p & 7)) & ((1 << dwidth) - 1)
                p += dwidth
                lengths_seen.add((symbol, extra))
                distances_seen.add((dsymbol, dextra))
                copy = (LENGTH_BASE[symbol] + extra, DIST_BASE[dsymbol] + dextra)
                if copy[1] > produced:
                    raise ValueError("scan: too far back")
                copies.add(copy)
                if copy == before:
                    repeats.add(copy)
                before = copy
                produced += copy[0]
                block["widest"] = max(block["widest"], p - first)
                if trace is not None:
                    trace += [("a length's extra bits", at - width, at), ("a distance code", at, p - dwidth), ("a distance's extra bits", p - dwidth, p),
                              ("a length and distance symbol", first, p)]
            block["lit_bits"] = {lit_lengths[k] for k in range(len(lit_lengths)) if seen[k]}
            block["dist_bits"] = {dist_lengths[k] for k in range(len(dist_lengths)) if dseen[k]}
        if p > 8 * n:
            raise ValueError("scan: the stream ends inside a block")
    return blocks, produced


def cut_inside(cdata: bytes, what: str, bits=None) -> bytes:
    """`cdata` up to the first byte boundary that lies inside a field `what` of `scan`'s trace (one of `bits` bits, if given)."""
    trace = []
    scan(cdata, trace)
    for kind, first, last in trace:
        cut = first // 8 * 8 + 8
        if kind == what and first < cut < last and bits in (None, last - first):
            return cdata[: cut // 8]
    raise AssertionError(f"no field '{what}' of this stream straddles a byte boundary")


def census(streams):
    """What the raw deflate streams make a decoder do, together: `lit_bits`, `dist_bits`, `cl_bits` (the code lengths decoded),
    `lengths` and `distances` ({(symbol, "zeros" or "ones")}: a symbol without extra bits counts as both), `through` (the
    symbols 258 came through: 284, 285), `pairs` (the ordered pairs of block kinds that follow each other inside a stream),
    `stored` ({(span offset of LEN, LEN)}), `copies` and `repeats` ({(length, distance)}), `widest` (the bits of the longest
    length and distance symbol), `cl_sets` (the lengths of each code-length code, as frozensets)."""
    total = dict(lit_bits=set(), dist_bits=set(), cl_bits=set(), lengths=set(), distances=set(), through=set(), pairs=set(), stored=set(),
                 copies=set(), repeats=set(), widest=0, cl_sets=set())
    for cdata in streams:
        blocks, _ = scan(cdata)
        for block in blocks:
            total["widest"] = max(total["widest"], block["widest"])
            total["cl_sets"].add(frozenset(block["cl_bits"]))
            for name in ("lit_bits", "dist_bits", "cl_bits", "copies", "repeats"):
                total[name] |= block[name]
            for name, widths in (("lengths", LENGTH_EXTRA), ("distances", DIST_EXTRA)):
                total[name] |= {(s, "zeros") for s, extra in block[name] if extra == 0}
                total[name] |= {(s, "ones") for s, extra in block[name] if extra == (1 << widths[s]) - 1}
            total["through"] |= {284 for pair in block["lengths"] if pair == (27, 31)} | {285 for s, _ in block["lengths"] if s == 28}
            if block["stored"] is not None:
                total["stored"].add(block["stored"])
        total["pairs"] |= {(a["kind"], b["kind"]) for a, b in zip(blocks, blocks[1:])}
    return total


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
    lanes, edges = [], []
    for label, cdata, data in census_streams():  # (one file each; the lane copies and the staging sweep as one file of many blocks)
        if label.startswith("lane copies"):
            lanes.append(around(cdata, data))
        elif "with LEN at span offset" in label:
            edges.append(around(cdata, data))
        else:
            files.append((f"hand-assembled: {label}", around(cdata, data) + EOF_BLOCK))
    files.append((f"hand-assembled: lane copies at the distances {', '.join(map(str, LANE_DISTANCES))}, a block each", b"".join(lanes) + EOF_BLOCK))
    files.append(("hand-assembled: stored blocks of (LEN bytes) with LEN at the span offsets " +
                  ", ".join(f"{at} ({n})" for at, n in stage_edges()) + f", a block each; staging windows of {stage_bytes()} bytes",
                  b"".join(edges) + EOF_BLOCK))
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


def cut_blocks():
    """[(label, one BGZF block that must be refused, ERR_STREAM)]: spans that end inside a field of a sound stream (`cut_inside`;
    what zlib says of each is the reason `verify` asks of the decoder)."""
    data = text_bytes(3000, 9)
    good = deflate(data)
    out = []
    for what in ("a distance code", "a distance's extra bits", "a repeat code's extra bits", "the HLIT / HDIST / HCLEN word", "the code-length code's lengths"):
        out.append((f"the span ends inside {what}", around(cut_inside(good, what), data), ERR_STREAM))
    (cdata, symbols), = [(cdata, says) for label, cdata, says in census_streams() if label.startswith("every length symbol")]
    out.append(("the span ends inside a length's extra bits", around(cut_inside(cdata, "a length's extra bits"), symbols), ERR_STREAM))
    out.append(("the span ends inside a stored LEN / NLEN", around(cut_inside(deflate(data, level=0), "a stored LEN / NLEN"), data), ERR_STREAM))
    label, cdata, long_data = census_streams()[0]
    first = len(cut_inside(cdata, "a length and distance symbol", bits=48))  # (the first byte boundary inside the first such symbol)
    for k in (0, 1, 4):
        out.append((f"the long-code stream cut at the byte boundary {k + 1} of its first 48-bit symbol", around(cdata[: first + k], long_data), ERR_STREAM))
    for k in (1, 2, 8):  # (its last symbol is one of 48 bits, the end-of-block code behind it one of 14)
        out.append((f"the long-code stream cut {k} bytes short", around(cdata[:-k], long_data), ERR_STREAM))
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
    files += [(label, sound[0] + bad + sound[1] + EOF_BLOCK, 1, code) for label, bad, code in cut_blocks()]
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


MUTATIONS_LONG = 2500  # (zlib accepts 4 of the first 1 000 and 13 of these: such a mutation must fall into bits no rule reads)
_mutations_long = None


def mutation_file_long():
    """One file of MUTATIONS_LONG blocks (its own seed): the same one-byte and one-bit mutations, of the streams of
    `census_streams()` alone, every one of them."""
    global _mutations_long
    if _mutations_long is not None:
        return _mutations_long
    rng = np.random.default_rng(2026)
    bases = [(cdata, data) for _, cdata, data in census_streams()]
    out = []
    for _ in range(MUTATIONS_LONG):
        cdata, data = bases[int(rng.integers(0, len(bases)))]
        changed = bytearray(cdata)
        at = int(rng.integers(0, len(changed)))
        if rng.random() < 0.5:
            changed[at] ^= 1 << int(rng.integers(0, 8))
        else:
            changed[at] = int(rng.integers(0, 256))
        out.append(around(bytes(changed), data))
    _mutations_long = b"".join(out)
    return _mutations_long


# ---- the period of the launch-turn test ------------------------------------------------------------------------------------------
def first_kind(span: bytes) -> str:
    """The kind of a span's first deflate block: s, f, d (a fixed or a dynamic block begins by building tables), or 3."""
    return "sfd3"[span[0] >> 1 & 3]


def turn_period():
    """(the bytes of a file of 15 small blocks, the indexes of those refused half-way): the period that the launch-turn test
    tiles past ROCCO_BGZF_MAX_GRID rows.  A workgroup's next block is row i + cap, so in the tiled table the block at index p of
    the period is followed, in its workgroup, by the one at (p + cap % 15) % 15.  The blocks are listed below in THAT order
    and placed accordingly: sound ones of every kind and refused ones of every verdict, and behind each block that is refused
    half-way -- with tables in LDS that it built and stopped using in mid-stream -- one that builds tables of its own:
      a dynamic block cut inside a length and distance symbol (both sets built, codes of up to 15 bits) -> a dynamic block
        whose distance set has one code;
      a dynamic block cut inside its code lengths (the literal/length table still holds the code-length code) -> a dynamic
        block with codes too long for the first-level tables (10 and 8 bits), decoded through the counts where the first-level
        table must hold 0 and not what was there before;
      a fixed block cut short -> a fixed block."""
    from math import gcd

    from rocco_amd import bam

    hand = {label: (cdata, data) for label, cdata, data in hand_streams() + census_streams()}
    text, records = text_bytes(90, 3), record_bytes(60)
    # literals in 1 .. 13 bits, 256 in 14, 284 in 15, distance symbol 9 in 10
    lit = lengths(286, **{f"s{65 + k}": k + 1 for k in range(13)}, s256=14, s284=15, s285=15)
    dist = list(range(1, 15)) + [0] * 14 + [15, 15]
    lc, dc = canonical(lit), canonical(dist)
    long_codes = Bits().dynamic(1, lit, dist)
    for byte in 2 * bytes(range(65, 78)):
        long_codes.literal(byte, lc)
    long_codes = long_codes.pair(27, 0, 9, 0, lc, dc).end(lc).bytes()  # (the pair: 15 + 5 + 10 + 3 bits, the end: 14)
    long_data = zlib.decompress(long_codes, wbits=-15)
    assert len(long_data) == 26 + 227
    repeats, repeats_data = hand["repeat codes 16, 17, 18 across the literal/distance boundary"]
    fixed = deflate(text[:40], strategy=zlib.Z_FIXED)
    chain = [("s", packed(records, level=0)),
             ("3", around(Bits().header(1, 3).bytes(), b"abc")),                                                  # refused: block type 3
             ("d", packed(text, level=9)),
             ("d", around(long_codes[:-3], long_data)),                                                           # refused half-way
             ("d", around(*hand["a distance set of one code, used"])),
             ("d", block(deflate(text), zlib.crc32(text), len(text) - 1)),                                        # refused: length
             ("f", EOF_BLOCK),                                                                                    # empty
             ("d", around(cut_inside(repeats, "a repeat code's extra bits"), repeats_data)),                      # refused half-way
             ("d", around(long_codes, long_data)),
             ("s", block(deflate(records, level=0), zlib.crc32(records) ^ 0x80, len(records))),                   # refused: CRC32
             ("d", around(*hand["a literal/length set of one code, an empty distance set"])),
             ("f", around(fixed[: len(fixed) // 2], text[:40])),                                                  # refused half-way
             ("f", packed(text[:40], strategy=zlib.Z_FIXED)),
             ("d", around(*hand["a code-length code with lengths 1 to 7"])),
             ("d", around(repeats, repeats_data))]
    half_way = (3, 7, 11)
    n = len(chain)
    step = bam.BGZF_MAX_GRID % n
    assert n % 2 == 1 and gcd(step, n) == 1  # (every block of the period is some workgroup's next after every other turn)
    blocks, placed = [None] * n, []
    for j, (kind, one) in enumerate(chain):
        blocks[j * step % n] = one
        assert first_kind(one[18:]) == kind, j  # (a block without extra subfields: its deflate data begins at byte 18)
        if j in half_way:
            placed.append(j * step % n)
    return b"".join(blocks), sorted(placed)


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


def stream_reason(span: bytes) -> str:
    """zlib's own words for a span it refuses: the tail of its message behind "data: "."""
    try:
        zlib.decompress(span, wbits=-15)
    except zlib.error as exc:
        text = str(exc)
        assert "data: " in text, text
        return text[text.index("data: ") + 6:]
    raise AssertionError("zlib accepts this span")


def expected_statuses(raw: bytes) -> np.ndarray:
    """The int32 status word per block: the verdict of `outcomes`, and for a stream error the number of zlib's reason
    (`rocco_amd.bam._STREAM_REASON_TEXT`) in bits 8 and up."""
    from rocco_amd import bam

    number = {text: why for why, text in bam._STREAM_REASON_TEXT.items()}
    rows = blocks_of(raw)
    return np.asarray([code | (number[stream_reason(raw[rows[k][1]: rows[k][2]])] << 8 if code == ERR_STREAM else 0)
                       for k, (code, _) in enumerate(outcomes(raw))], dtype=np.int32)


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
    """`status` and `out` (filled with GUARD_BYTE before the call) against `outcomes(raw)`: every block's status code, for a
    stream error the reason in zlib's own words for that span (`stream_reason`; no reason with any other verdict), the bytes of
    every accepted block, and not one byte changed outside the blocks' ranges.  Returns the index of the first refused block
    or -1."""
    from rocco_amd import bam

    want = outcomes(raw)
    rows = blocks_of(raw)
    assert len(want) == table.shape[0] == status.shape[0], label
    inside = np.zeros(out.shape[0], dtype=bool)
    first = -1
    for k, (code, data) in enumerate(want):
        at, isize = int(table[k, 4]), int(table[k, 2])
        inside[at: at + isize] = True
        assert int(status[k]) & 0xFF == code, (label, k, int(status[k]), code)
        if code == ERR_STREAM:
            says, zlib_says = bam._STREAM_REASON_TEXT.get(int(status[k]) >> 8), stream_reason(raw[rows[k][1]: rows[k][2]])
            assert says == zlib_says, (label, k, int(status[k]), says, zlib_says)
        else:
            assert int(status[k]) >> 8 == 0, (label, k, int(status[k]), code)
        if code == 0:
            assert out[at: at + isize].tobytes() == data, (label, k)
        elif first < 0:
            first = k
    assert np.all(out[~inside] == GUARD_BYTE), (label, "a byte outside the blocks' ranges was written")
    return first
