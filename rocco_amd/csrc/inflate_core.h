// rocco_amd/csrc/inflate_core.h -- RFC 1951 inflate of one block and its check value under BGZF or zlib framing: ONE statement
// of the decode rules, compiled for the device (csrc/bgzf_inflate.hip: one wavefront per block) and for the host (inflate_host
// below: one thread, test support in the sense synth.hip is).  DESIGN.md section 0 rows f8 and f10, notes (29) and (31).
//
// The code is written for L lanes that all carry the same decoder state (bit buffer, output position, current tables) and
// branch alike; what differs between lanes is only which element of a cooperative loop a lane takes: the symbols of a code
// set when its tables are built, the bytes of a match or a stored block when they are copied.  The executor X says what a
// lane is:
//   X::kLanes, x.lane()    64 and the lane on the device; 1 and 0 on the host
//   x.ballot(p)            the lanes where p holds, as a bit mask
//   x.sync()               every store made so far by any lane (tables, output bytes) is visible to every lane
//   x.in_byte(i)           byte i of the compressed buffer; the core asks only for lo <= i < hi, the block's span
//   x.in_raw(i)            the same without staging (the bytes of a stored block, read once, one per lane)
//
// Acceptance is zlib 1.2.11's inflate() over a raw stream (`zlib.decompress(span, wbits=-15)`), rule by rule:
//   block type 3 is rejected; a stored LEN must equal ~NLEN; HLIT <= 286 and HDIST <= 30; the code-length code must be
//   complete; a repeat code may not run past HLIT + HDIST lengths and a leading 16 is rejected; symbol 256 needs a code; an
//   over-subscribed literal/length or distance set is rejected; an incomplete one too, except a set with exactly one code of
//   length 1 and an empty distance set; using a code such a set lacks is an error, as are the fixed code's literal/length
//   symbols 286 and 287 and distance symbols 30 and 31; a distance beyond the bytes produced so far is rejected; input that
//   ends before the final block ends is rejected (bits are asked for exactly when a symbol needs them); what follows the
//   final block inside the span is ignored.
// zlib knows no ISIZE: a stream that inflates to more than the block's ISIZE is decoded to its end all the same, counting
// and not storing, so that a stream that is too long AND corrupt further on is reported as zlib reports it (a stream
// error), and a sound one as a length error.  Every store is bounded by ISIZE, every load by the span.
#pragma once

#include <stdint.h>

#include "../../include/rocco_hip.h"

#if defined(__HIPCC__)
#define ROCCO_INFLATE_HD __host__ __device__ inline
#else
#define ROCCO_INFLATE_HD inline
#endif

namespace rocco {

constexpr int kInflateMaxBits = 15;
constexpr int kInflateLitSymbols = 288, kInflateDistSymbols = 32, kInflateLitFastBits = 10, kInflateDistFastBits = 8;
constexpr int kInflateMaxLengths = 320;  // HLIT + HDIST <= 286 + 30, and the 288 + 32 of the fixed code

// the sub-reason of ROCCO_BGZF_ERR_STREAM, in bits 8..15 of a status word
enum InflateWhy {
    kInflateBlockType = 1, kInflateStoredLength, kInflateTooManySymbols, kInflateCodeLengthsSet, kInflateRepeat, kInflateNoEndOfBlock,
    kInflateLiteralSet, kInflateDistanceSet, kInflateLiteralCode, kInflateDistanceCode, kInflateTooFarBack, kInflateTruncated,
};
static_assert(kInflateTruncated == ROCCO_BGZF_STREAM_REASONS, "rocco_hip.h states the reasons");

ROCCO_INFLATE_HD int inflate_stream_error(int why) { return ROCCO_BGZF_ERR_STREAM | (why << 8); }

// A canonical Huffman code: count[l] codes of length l, the symbols ordered by (length, symbol), and a first-level table over
// the next F bits of the stream: (symbol << 4 | length) where a code of length <= F begins there, 0 where none does (a longer
// code, or a code the set lacks: both go through the counts).
template <int N, int F>
struct HuffTable {
    static constexpr int kSymbols = N, kFastBits = F;
    uint16_t count[kInflateMaxBits + 1];
    uint16_t symbol[N];
    uint16_t fast[1 << F];
};

struct InflateTables {
    HuffTable<kInflateLitSymbols, kInflateLitFastBits> lit;  // (also the code-length code while a dynamic header is read)
    HuffTable<kInflateDistSymbols, kInflateDistFastBits> dist;
    uint8_t lens[kInflateMaxLengths];
};

struct InflateBits {
    uint64_t hold;  // the next `bits` bits of the stream, the first in bit 0; zero above them
    int bits;
    long long ip, hi;  // the next byte to fetch; one past the span
};

template <class X>
ROCCO_INFLATE_HD void inflate_refill(X &x, InflateBits &b)
{
    while (b.bits <= 56 && b.ip < b.hi) {
        b.hold |= (uint64_t)x.in_byte(b.ip++) << b.bits;
        b.bits += 8;
    }
}

// n <= 32 bits that the caller knows to be there
ROCCO_INFLATE_HD uint32_t inflate_take(InflateBits &b, int n)
{
    const uint32_t v = (uint32_t)(b.hold & ((1ULL << n) - 1ULL));
    b.hold >>= n;
    b.bits -= n;
    return v;
}

// Builds h from lens[0, n): > 0 the set is incomplete (the codes left over, in units of 2^-15), 0 complete, < 0
// over-subscribed (h is then unusable).  Cooperative: a lane takes the symbols lane, lane + L, ...; per length the lanes
// that hold a symbol of it are counted and ranked with one ballot, which sorts the symbols and counts them in one pass.
template <class X, class H>
ROCCO_INFLATE_HD int huff_build(X &x, H &h, const uint8_t *lens, int n)
{
    const int lane = x.lane();
    const uint64_t below = (1ULL << lane) - 1ULL;
    x.sync();  // (lens are written; nobody still reads the tables of the block before)
    for (int k = lane; k < (1 << H::kFastBits); k += X::kLanes) {
        h.fast[k] = 0;
    }
    int at = 0, left = 1;
    bool over = false;
    for (int l = 1; l <= kInflateMaxBits; ++l) {
        const int begin = at;
        for (int base = 0; base < n; base += X::kLanes) {
            const int s = base + lane;
            const bool mine = s < n && lens[s] == l;
            const uint64_t who = x.ballot(mine);
            if (mine) {
                h.symbol[at + __builtin_popcountll(who & below)] = (uint16_t)s;
            }
            at += __builtin_popcountll(who);
        }
        h.count[l] = (uint16_t)(at - begin);  // (every lane stores the same value)
        left = (left << 1) - (at - begin);
        if (left < 0) {
            over = true;
            break;
        }
    }
    h.count[0] = (uint16_t)(n - at);
    if (over) {
        return -1;
    }
    x.sync();  // (symbol[] and the cleared fast[] are whole)
    // the first-level table: the lane's share of the sorted symbols; code j of length l is first(l) + its rank, where
    // first(l) = (first(l - 1) + count[l - 1]) << 1; the stream holds a code's bits most significant first
    for (int j = lane; j < at; j += X::kLanes) {
        int l = 1, first = 0, index = 0;
        while (j >= index + h.count[l]) {
            index += h.count[l];
            first = (first + h.count[l]) << 1;
            ++l;
        }
        if (l <= H::kFastBits) {
            const uint32_t code = (uint32_t)(first + (j - index));
            uint32_t rev = 0;
            for (int k = 0; k < l; ++k) {
                rev |= ((code >> k) & 1u) << (l - 1 - k);
            }
            const uint16_t entry = (uint16_t)((h.symbol[j] << 4) | l);
            for (uint32_t k = rev; k < (1u << H::kFastBits); k += 1u << l) {
                h.fast[k] = entry;
            }
        }
    }
    x.sync();
    return left;
}

// The next symbol of h: 0, or why not.  Consumes the code's bits: at least one.
template <class H>
ROCCO_INFLATE_HD int huff_decode(const H &h, InflateBits &b, int invalid, int *symbol_out)
{
    const uint32_t peek = (uint32_t)b.hold;  // (zeros behind the stream's end)
    const uint32_t entry = h.fast[peek & ((1u << H::kFastBits) - 1u)];
    int len = 0, symbol = 0;
    if (entry != 0) {
        len = (int)(entry & 15u);
        symbol = (int)(entry >> 4);
    } else {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l <= kInflateMaxBits; ++l) {
            code |= (int)((peek >> (l - 1)) & 1u);
            const int count = h.count[l];
            if (code - count < first) {
                symbol = h.symbol[index + (code - first)];
                len = l;
                break;
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        if (len == 0) {
            return invalid;  // (no code of the set begins with these bits)
        }
    }
    if (len > b.bits) {
        return kInflateTruncated;
    }
    b.hold >>= len;
    b.bits -= len;
    *symbol_out = symbol;
    return 0;
}

// Inflates the span [lo, hi) of the compressed buffer into out[0, isize).  Returns 0, ROCCO_BGZF_ERR_STREAM | why << 8, or
// ROCCO_BGZF_ERR_LENGTH; *produced_out: the bytes the stream inflates to (where it is sound); *end_out (may be null, as the
// BGZF callers leave it): where a sound stream ended in the compressed buffer -- the byte behind the last bit of its final
// block, the bit reader rounded up to a byte (what zlib's framing keeps its check value at).
template <class X>
ROCCO_INFLATE_HD int inflate_block(X &x, InflateTables &t, long long lo, long long hi, uint8_t *out, long long isize, long long *produced_out,
                                   long long *end_out = nullptr)
{
    const int lane = x.lane();
    InflateBits b = {0, 0, lo, hi};
    long long pos = 0;     // bytes produced; those at isize and beyond are counted, not stored
    long long fenced = 0;  // out[0, fenced) is visible to every lane (x.sync() ran when pos was there)
    *produced_out = 0;
    // Termination: every pass of the three loops below (deflate blocks, code lengths, symbols) consumes at least one bit of
    // the span or returns -- a block header is 3 bits, huff_decode hands out a symbol only with its code's bits (>= 1) -- and
    // no bit is handed out twice, so a corrupt span ends after at most 8 (hi - lo) passes in all: there is no loop cap.
    for (;;) {
        inflate_refill(x, b);
        if (b.bits < 3) {
            return inflate_stream_error(kInflateTruncated);
        }
        const uint32_t last = inflate_take(b, 1), type = inflate_take(b, 2);
        if (type == 3) {
            return inflate_stream_error(kInflateBlockType);
        }
        if (type == 0) {
            (void)inflate_take(b, b.bits & 7);
            inflate_refill(x, b);
            if (b.bits < 32) {
                return inflate_stream_error(kInflateTruncated);
            }
            const uint32_t len = inflate_take(b, 16), nlen = inflate_take(b, 16);
            if (len != (~nlen & 0xffffu)) {
                return inflate_stream_error(kInflateStoredLength);
            }
            b.ip -= b.bits >> 3;  // (whole bytes are buffered: hand them back, the copy reads the buffer itself)
            b.hold = 0;
            b.bits = 0;
            if (b.ip + (long long)len > hi) {
                return inflate_stream_error(kInflateTruncated);
            }
            for (long long k = lane; k < (long long)len; k += X::kLanes) {
                if (pos + k < isize) {
                    out[pos + k] = x.in_raw(b.ip + k);
                }
            }
            pos += len;
            b.ip += len;
        } else {
            if (type == 1) {
                for (int s = lane; s < kInflateLitSymbols + kInflateDistSymbols; s += X::kLanes) {
                    t.lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : (s < 288 ? 8 : 5))));
                }
                (void)huff_build(x, t.lit, t.lens, kInflateLitSymbols);  // (complete; 286 and 287 are refused where they come up)
                (void)huff_build(x, t.dist, t.lens + kInflateLitSymbols, kInflateDistSymbols);  // (complete; 30 and 31 likewise)
            } else {
                if (b.bits < 14) {
                    return inflate_stream_error(kInflateTruncated);
                }
                const int nlen = (int)inflate_take(b, 5) + 257, ndist = (int)inflate_take(b, 5) + 1, ncode = (int)inflate_take(b, 4) + 4;
                if (nlen > 286 || ndist > 30) {
                    return inflate_stream_error(kInflateTooManySymbols);
                }
                for (int k = 0; k < 19; ++k) {  // (every lane stores the same values)
                    // the order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                    const int where = k < 3 ? 16 + k : (k == 3 ? 0 : ((k & 1) ? 8 - ((k - 3) >> 1) : 8 + ((k - 4) >> 1)));
                    uint32_t v = 0;
                    if (k < ncode) {
                        inflate_refill(x, b);
                        if (b.bits < 3) {
                            return inflate_stream_error(kInflateTruncated);
                        }
                        v = inflate_take(b, 3);
                    }
                    t.lens[where] = (uint8_t)v;
                }
                if (huff_build(x, t.lit, t.lens, 19) != 0) {
                    return inflate_stream_error(kInflateCodeLengthsSet);
                }
                int have = 0, before = 0;
                bool end_of_block = false;
                while (have < nlen + ndist) {
                    inflate_refill(x, b);
                    int symbol = 0;
                    if (const int why = huff_decode(t.lit, b, kInflateCodeLengthsSet, &symbol); why != 0) {
                        return inflate_stream_error(why);
                    }
                    int repeat = 1, value = symbol;
                    if (symbol >= 16) {
                        const int extra = symbol == 16 ? 2 : (symbol == 17 ? 3 : 7);
                        if (symbol == 16 && have == 0) {
                            return inflate_stream_error(kInflateRepeat);
                        }
                        if (b.bits < extra) {
                            return inflate_stream_error(kInflateTruncated);
                        }
                        repeat = (symbol == 18 ? 11 : 3) + (int)inflate_take(b, extra);
                        value = symbol == 16 ? before : 0;
                        if (have + repeat > nlen + ndist) {
                            return inflate_stream_error(kInflateRepeat);
                        }
                    }
                    // (the lengths land behind the code-length code's 19, which huff_decode no longer needs: it reads h)
                    for (int k = 0; k < repeat; ++k) {
                        t.lens[have + k] = (uint8_t)value;
                    }
                    if (value != 0 && have <= 256 && 256 < have + repeat) {
                        end_of_block = true;
                    }
                    have += repeat;
                    before = value;
                }
                if (!end_of_block) {
                    return inflate_stream_error(kInflateNoEndOfBlock);
                }
                // an incomplete set passes only as one code of length 1 (or, for the distances, as no code at all)
                const int lit_left = huff_build(x, t.lit, t.lens, nlen);
                if (lit_left < 0 || (lit_left > 0 && nlen != t.lit.count[0] + t.lit.count[1])) {
                    return inflate_stream_error(kInflateLiteralSet);
                }
                const int dist_left = huff_build(x, t.dist, t.lens + nlen, ndist);
                if (dist_left < 0 || (dist_left > 0 && ndist != t.dist.count[0] + t.dist.count[1])) {
                    return inflate_stream_error(kInflateDistanceSet);
                }
            }
            for (;;) {
                inflate_refill(x, b);  // (57 bits or the span's rest: a length and a distance with their extra bits are 48 at most)
                int symbol = 0;
                if (const int why = huff_decode(t.lit, b, kInflateLiteralCode, &symbol); why != 0) {
                    return inflate_stream_error(why);
                }
                if (symbol < 256) {
                    if (lane == 0 && pos < isize) {
                        out[pos] = (uint8_t)symbol;
                    }
                    ++pos;
                    continue;
                }
                if (symbol == 256) {
                    break;
                }
                symbol -= 257;
                if (symbol >= 29) {
                    return inflate_stream_error(kInflateLiteralCode);
                }
                // lengths 3 .. 258: eight without extra bits, then four per number of extra bits, 258 on its own
                const int len_extra = symbol < 8 || symbol == 28 ? 0 : (symbol >> 2) - 1;
                if (b.bits < len_extra) {
                    return inflate_stream_error(kInflateTruncated);
                }
                const long long len = symbol == 28 ? 258 : (symbol < 8 ? 3 + symbol : 3 + ((4 + (symbol & 3)) << len_extra) + (int)inflate_take(b, len_extra));
                int dsym = 0;
                if (const int why = huff_decode(t.dist, b, kInflateDistanceCode, &dsym); why != 0) {
                    return inflate_stream_error(why);
                }
                if (dsym >= 30) {
                    return inflate_stream_error(kInflateDistanceCode);
                }
                // distances 1 .. 32768: four without extra bits, then two per number of extra bits
                const int dist_extra = dsym < 4 ? 0 : (dsym >> 1) - 1;
                if (b.bits < dist_extra) {
                    return inflate_stream_error(kInflateTruncated);
                }
                const long long dist = dsym < 4 ? 1 + dsym : 1 + ((2 + (dsym & 1)) << dist_extra) + (long long)inflate_take(b, dist_extra);
                if (dist > pos) {
                    return inflate_stream_error(kInflateTooFarBack);
                }
                // out[pos + k] = out[pos - dist + k mod dist]: every source byte lies below pos, so the lanes copy side by side
                // whatever the overlap; the source must be visible to them first
                const long long from = pos - dist;
                if (from + (dist < len ? dist : len) > fenced) {
                    x.sync();
                    fenced = pos;
                }
                for (long long k = lane; k < len; k += X::kLanes) {
                    if (pos + k < isize) {  // (the source index is smaller still)
                        out[pos + k] = out[from + (k < dist ? k : k % dist)];
                    }
                }
                pos += len;
            }
        }
        if (last) {
            break;
        }
    }
    *produced_out = pos;
    if (end_out != nullptr) {
        *end_out = b.ip - (b.bits >> 3);  // (the whole bytes still buffered were fetched and not used)
    }
    return pos == isize ? 0 : ROCCO_BGZF_ERR_LENGTH;
}

// ---- CRC32 (the gzip polynomial, reflected) ------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr int kCrcChunks = 64;  // a block's bytes are cut into this many contiguous chunks, one per lane on the device

struct CrcTables {
    uint32_t byte[256];  // the CRC of one byte
    uint32_t x2n[32];    // x^(2^k) modulo the polynomial
};

// a(x) b(x) modulo the polynomial (zlib's multmodp)
ROCCO_INFLATE_HD uint32_t crc_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) {
                break;
            }
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

ROCCO_INFLATE_HD uint32_t crc_byte_entry(uint32_t n)
{
    for (int k = 0; k < 8; ++k) {
        n = (n & 1u) ? kCrcPoly ^ (n >> 1) : n >> 1;
    }
    return n;
}

// the lane's share of both tables (x2n is a chain of squarings: every lane computes its own entry from x^1)
template <class X>
ROCCO_INFLATE_HD void crc_tables_build(X &x, CrcTables &t)
{
    for (int k = x.lane(); k < 256; k += X::kLanes) {
        t.byte[k] = crc_byte_entry((uint32_t)k);
    }
    for (int k = x.lane(); k < 32; k += X::kLanes) {
        uint32_t p = 1u << 30;
        for (int j = 0; j < k; ++j) {
            p = crc_multmodp(p, p);
        }
        t.x2n[k] = p;
    }
    x.sync();
}

ROCCO_INFLATE_HD uint32_t crc_of_bytes(const CrcTables &t, const uint8_t *p, long long n)
{
    uint32_t c = 0xffffffffu;
    for (long long k = 0; k < n; ++k) {
        c = t.byte[(c ^ p[k]) & 0xffu] ^ (c >> 8);
    }
    return ~c;
}

// the CRC of A || B from the CRCs of A and B and B's length (zlib's crc32_combine: crc(A) x^(8 len B) + crc(B))
ROCCO_INFLATE_HD uint32_t crc_combine(const CrcTables &t, uint32_t crc_a, uint32_t crc_b, long long len_b)
{
    uint32_t p = 1u << 31;
    for (unsigned k = 3; len_b != 0; len_b >>= 1, ++k) {
        if (len_b & 1) {
            p = crc_multmodp(t.x2n[k & 31u], p);
        }
    }
    return crc_multmodp(p, crc_a) ^ crc_b;
}

// chunk c of kCrcChunks of n bytes: [first, first + length)
ROCCO_INFLATE_HD void crc_chunk(long long n, int c, long long *first, long long *length)
{
    const long long each = (n + kCrcChunks - 1) / kCrcChunks, lo = each * c < n ? each * c : n, hi = lo + each < n ? lo + each : n;
    *first = lo;
    *length = hi - lo;
}

// ---- a framing: what stands around the deflate data of a row, as a compile-time policy of the kernels (bgzf_inflate.hip) and
// of their host twin (inflate_host below).  F states the table (kColumns, kOffsetColumn: where the row's bytes go in the output
// buffer), the grid cap, fits(row, n_comp, n_out) (the row against the two buffers) and block(x, tables, row, out, &produced,
// &end) (everything of the row but its check value); and for the check: has_check(row), check_bytes(row, produced) (the bytes
// it covers), check_chunk / check_combine / kCheckStart (a chunk's value, the value of A || B, the value of no bytes),
// stated(row, comp, end) (the value the file states), kCheckError, CheckTables with check_tables_build (what the chunk
// function looks up, in LDS on the device), and kStatedInStream: the stated value is read from the compressed buffer at the
// stream's end (the kernels then keep an `ends` array and the check reads comp) instead of from the row.

// BGZF (rocco_hip.h: row = first, last, ISIZE, CRC32, offset): a raw deflate stream that inflates to exactly ISIZE bytes
struct BgzfFraming {
    static constexpr int kColumns = ROCCO_BGZF_TABLE_COLUMNS, kOffsetColumn = 4, kCheckError = ROCCO_BGZF_ERR_CRC;
    static constexpr long long kMaxGrid = ROCCO_BGZF_MAX_GRID;
    static constexpr bool kStatedInStream = false;
    static constexpr uint32_t kCheckStart = 0;
    using CheckTables = CrcTables;

    static ROCCO_INFLATE_HD bool fits(const int64_t *row, long long n_comp, long long n_out)
    {
        return row[0] >= 0 && row[0] <= row[1] && row[1] <= n_comp && row[2] >= 0 && row[2] <= ROCCO_BGZF_MAX_ISIZE && row[4] >= 0 &&
               row[4] <= n_out && row[2] <= n_out - row[4];
    }
    template <class X>
    static ROCCO_INFLATE_HD int block(X &x, InflateTables &t, const int64_t *row, uint8_t *out, long long *produced_out, long long *)
    {
        return inflate_block(x, t, row[0], row[1], out, row[2], produced_out);
    }
    static ROCCO_INFLATE_HD bool has_check(const int64_t *) { return true; }
    static ROCCO_INFLATE_HD long long check_bytes(const int64_t *row, long long) { return row[2]; }
    template <class X>
    static ROCCO_INFLATE_HD void check_tables_build(X &x, CrcTables &t) { crc_tables_build(x, t); }
    static ROCCO_INFLATE_HD uint32_t check_chunk(const CrcTables &t, const uint8_t *p, long long n) { return crc_of_bytes(t, p, n); }
    static ROCCO_INFLATE_HD uint32_t check_combine(const CrcTables &t, uint32_t a, uint32_t b, long long len_b) { return crc_combine(t, a, b, len_b); }
    static ROCCO_INFLATE_HD uint32_t stated(const int64_t *row, const uint8_t *, long long) { return (uint32_t)row[3]; }
};

// ---- the host entry (test support): one thread, the same functions ---------------------------------------------------------
struct HostInflateExec {
    static constexpr int kLanes = 1;
    const uint8_t *comp;
    int lane() const { return 0; }
    uint64_t ballot(bool p) const { return p ? 1u : 0u; }
    void sync() const {}
    uint32_t in_byte(long long i) const { return comp[i]; }
    uint8_t in_raw(long long i) const { return comp[i]; }
};

// What the two kernels of bgzf_inflate.hip compute under framing F, block after block: status_out[i] and produced_out[i]
// (either may be null), the bytes of every block at its offset, and report_out[ROCCO_BGZF_REPORT] = the first failing block
// (-1), its status, the bytes it inflates to, 0.
template <class F>
inline void inflate_host(const uint8_t *comp, long long n_comp, const int64_t *table, long long n_blocks, uint8_t *out, long long n_out,
                         int32_t *status_out, int64_t *produced_out, int64_t *report_out)
{
    HostInflateExec x = {comp};
    InflateTables tables;
    typename F::CheckTables check_tables;
    F::check_tables_build(x, check_tables);
    report_out[0] = -1;
    report_out[1] = report_out[2] = report_out[3] = 0;
    for (long long i = 0; i < n_blocks; ++i) {
        const int64_t *row = table + i * F::kColumns;
        int status = ROCCO_BGZF_ERR_TABLE;
        long long produced = 0, end = 0;
        if (F::fits(row, n_comp, n_out)) {
            uint8_t *mine = out + row[F::kOffsetColumn];
            status = F::block(x, tables, row, mine, &produced, &end);
            if (status == 0 && F::has_check(row)) {
                uint32_t check = F::kCheckStart;
                for (int c = 0; c < kCrcChunks; ++c) {
                    long long first, length;
                    crc_chunk(F::check_bytes(row, produced), c, &first, &length);
                    check = F::check_combine(check_tables, check, F::check_chunk(check_tables, mine + first, length), length);
                }
                status = check == F::stated(row, comp, end) ? 0 : F::kCheckError;
            }
        }
        if (status_out != nullptr) {
            status_out[i] = status;
        }
        if (produced_out != nullptr) {
            produced_out[i] = produced;
        }
        if (status != 0 && report_out[0] < 0) {
            report_out[0] = i;
            report_out[1] = status;
            report_out[2] = produced;
        }
    }
}

// ---- zlib framing (RFC 1950) around the same deflate data: the data blocks of a bigWig file (note (31)) ------
// Two header bytes, the deflate stream, the Adler-32 of the inflated bytes in four big-endian bytes.  Acceptance is zlib
// 1.2.11's inflate() with wbits = 15 as uncompress() drives it, in the order in which it would meet the faults.
constexpr uint32_t kAdlerBase = 65521u;  // the largest prime below 2^16
constexpr int kAdlerDefer = 5552;        // zlib's NMAX: the bytes whose sums fit 32 bits before a reduction
enum ZlibHeaderWhy { kZlibHeaderCheck = 1, kZlibMethod, kZlibWindow, kZlibDictionary };
static_assert(kZlibDictionary == ROCCO_ZLIB_HEADER_REASONS, "rocco_hip.h states the reasons");

// the two header bytes: 0, or ROCCO_ZLIB_ERR_HEADER | why << 8
ROCCO_INFLATE_HD int zlib_header_status(uint32_t cmf, uint32_t flg)
{
    if (((cmf << 8) + flg) % 31u != 0) {
        return ROCCO_ZLIB_ERR_HEADER | (kZlibHeaderCheck << 8);
    }
    if ((cmf & 15u) != 8u) {
        return ROCCO_ZLIB_ERR_HEADER | (kZlibMethod << 8);
    }
    if ((cmf >> 4) > 7u) {
        return ROCCO_ZLIB_ERR_HEADER | (kZlibWindow << 8);
    }
    return (flg & 0x20u) ? ROCCO_ZLIB_ERR_HEADER | (kZlibDictionary << 8) : 0;
}

// the Adler-32 of n bytes on their own (zlib's adler32 from 1)
ROCCO_INFLATE_HD uint32_t adler_of_bytes(const uint8_t *p, long long n)
{
    uint32_t a = 1, b = 0;
    while (n > 0) {
        const int run = n < kAdlerDefer ? (int)n : kAdlerDefer;
        for (int k = 0; k < run; ++k) {
            a += p[k];
            b += a;
        }
        a %= kAdlerBase;
        b %= kAdlerBase;
        p += run;
        n -= run;
    }
    return (b << 16) | a;
}

// the Adler-32 of A || B from those of A and B and B's length (zlib's adler32_combine)
ROCCO_INFLATE_HD uint32_t adler_combine(uint32_t adler_a, uint32_t adler_b, long long len_b)
{
    const uint32_t rem = (uint32_t)(len_b % (long long)kAdlerBase);
    uint32_t sum1 = adler_a & 0xffffu;
    uint32_t sum2 = (rem * sum1) % kAdlerBase;
    sum1 += (adler_b & 0xffffu) + kAdlerBase - 1;
    sum2 += ((adler_a >> 16) & 0xffffu) + ((adler_b >> 16) & 0xffffu) + kAdlerBase - rem;
    if (sum1 >= kAdlerBase) {
        sum1 -= kAdlerBase;
    }
    if (sum1 >= kAdlerBase) {
        sum1 -= kAdlerBase;
    }
    if (sum2 >= (kAdlerBase << 1)) {
        sum2 -= kAdlerBase << 1;
    }
    if (sum2 >= kAdlerBase) {
        sum2 -= kAdlerBase;
    }
    return sum1 | (sum2 << 16);
}

// Everything of a row but its Adler-32: the header, the stream, the room for the check value, the length; a stored row is
// copied.  Returns the status so far (0: the Adler-32 of out[0, *produced_out) is still to be compared with the four bytes
// at *end_out; a stored row has none and *end_out is its span's end).  Cooperative, as inflate_block is.
template <class X>
ROCCO_INFLATE_HD int zlib_block(X &x, InflateTables &t, const int64_t *row, uint8_t *out, long long *produced_out, long long *end_out)
{
    const long long lo = row[0], hi = row[1], capacity = row[2];
    *produced_out = 0;
    *end_out = hi;
    if (row[4] == 1) {
        for (long long k = x.lane(); k < hi - lo && k < capacity; k += X::kLanes) {
            out[k] = x.in_raw(lo + k);
        }
        *produced_out = hi - lo;
        return hi - lo > capacity ? ROCCO_BGZF_ERR_LENGTH : 0;
    }
    if (hi - lo < 2) {
        return ROCCO_ZLIB_ERR_TRUNCATED;
    }
    if (const int bad = zlib_header_status(x.in_raw(lo), x.in_raw(lo + 1)); bad != 0) {
        // (zlib reads the dictionary's id before it asks for the dictionary: without its four bytes the input just ends)
        return (bad >> 8) == kZlibDictionary && hi - lo < 6 ? ROCCO_ZLIB_ERR_TRUNCATED : bad;
    }
    const int status = inflate_block(x, t, lo + 2, hi, out, capacity, produced_out, end_out);
    if ((status & 0xff) == ROCCO_BGZF_ERR_STREAM) {
        return status;
    }
    if (hi - *end_out < 4) {
        return ROCCO_ZLIB_ERR_TRUNCATED;
    }
    return *produced_out > capacity ? ROCCO_BGZF_ERR_LENGTH : 0;
}

ROCCO_INFLATE_HD uint32_t zlib_stated_adler(const uint8_t *comp, long long at)
{
    return ((uint32_t)comp[at] << 24) | ((uint32_t)comp[at + 1] << 16) | ((uint32_t)comp[at + 2] << 8) | (uint32_t)comp[at + 3];
}

// zlib (rocco_hip.h: row = first, last, capacity, offset, framing): the Adler-32 covers the bytes produced (at most the
// capacity) and stands behind the stream; a stored row (framing 1) has none
struct ZlibFraming {
    static constexpr int kColumns = ROCCO_ZLIB_TABLE_COLUMNS, kOffsetColumn = 3, kCheckError = ROCCO_ZLIB_ERR_ADLER;
    static constexpr long long kMaxGrid = ROCCO_ZLIB_MAX_GRID;
    static constexpr bool kStatedInStream = true;
    static constexpr uint32_t kCheckStart = 1;
    struct CheckTables {};  // (the Adler-32 looks nothing up)

    static ROCCO_INFLATE_HD bool fits(const int64_t *row, long long n_comp, long long n_out)
    {
        return row[0] >= 0 && row[0] <= row[1] && row[1] <= n_comp && row[2] >= 0 && row[2] <= ROCCO_BGZF_MAX_ISIZE && row[3] >= 0 &&
               row[3] <= n_out && row[2] <= n_out - row[3] && (row[4] == 0 || row[4] == 1);
    }
    template <class X>
    static ROCCO_INFLATE_HD int block(X &x, InflateTables &t, const int64_t *row, uint8_t *out, long long *produced_out, long long *end_out)
    {
        return zlib_block(x, t, row, out, produced_out, end_out);
    }
    static ROCCO_INFLATE_HD bool has_check(const int64_t *row) { return row[4] == 0; }
    static ROCCO_INFLATE_HD long long check_bytes(const int64_t *, long long produced) { return produced; }
    template <class X>
    static ROCCO_INFLATE_HD void check_tables_build(X &, CheckTables &) {}
    static ROCCO_INFLATE_HD uint32_t check_chunk(const CheckTables &, const uint8_t *p, long long n) { return adler_of_bytes(p, n); }
    static ROCCO_INFLATE_HD uint32_t check_combine(const CheckTables &, uint32_t a, uint32_t b, long long len_b) { return adler_combine(a, b, len_b); }
    static ROCCO_INFLATE_HD uint32_t stated(const int64_t *, const uint8_t *comp, long long end) { return zlib_stated_adler(comp, end); }
};

}  // namespace rocco
