// rocco_amd/csrc/bam_record.h -- the layout of one BAM alignment record in the inflated byte stream, and THE plausibility
// predicate of the record walk (note (29)).  tests/bam_expected.py restates both in NumPy, line
// for line; tests/golden/make_golden_bam_files.py uses that statement to know exactly what fools the guess.  Change one,
// change the other.
//
// A record at byte offset p (any alignment):
//   p +  0  int32  block_size   bytes that follow this word
//   p +  4  int32  refID        p + 12 uint8  l_read_name    p + 16 uint16 n_cigar_op    p + 24 int32 next_refID
//   p +  8  int32  pos          p + 13 uint8  mapq           p + 18 uint16 flag          p + 28 int32 next_pos
//                               p + 14 uint16 bin            p + 20 int32  l_seq         p + 32 int32 tlen
//   p + 36  read_name (l_read_name bytes), cigar (4 n_cigar_op), seq ((l_seq + 1) / 2), qual (l_seq), tags
// The next record begins at p + 4 + block_size.  Integers are little-endian and assembled from byte loads: a record lies
// at an arbitrary offset, and no pointer is cast.
#pragma once

#include <cstdint>

#include "../../include/rocco_hip.h"

#if defined(__HIPCC__)
#define ROCCO_BAM_FN __host__ __device__ __forceinline__
#else
#define ROCCO_BAM_FN inline
#endif

namespace rocco {

namespace {

constexpr int kBamFixed = 36;        // the block_size word and the 32 fixed bytes behind it
constexpr int kBamMinBlockSize = 32;
constexpr int kBamGuessDepth = ROCCO_BAM_GUESS_DEPTH;
constexpr long long kBamRunoff = ROCCO_BAM_RUNOFF_BYTES;

ROCCO_BAM_FN unsigned bam_u8(const uint8_t *b, long long o) { return (unsigned)b[o]; }
ROCCO_BAM_FN unsigned bam_u16(const uint8_t *b, long long o) { return bam_u8(b, o) | (bam_u8(b, o + 1) << 8); }
ROCCO_BAM_FN unsigned bam_u32(const uint8_t *b, long long o) { return bam_u16(b, o) | (bam_u16(b, o + 2) << 16); }
ROCCO_BAM_FN int bam_i32(const uint8_t *b, long long o) { return (int)bam_u32(b, o); }

// The header at b + o (its 36 bytes are the caller's to bound) could be a record's, for a file with n_ref contigs:
//   block_size >= 32; refID and next_refID in [-1, n_ref); l_read_name >= 1; l_seq >= 0;
//   4 n_cigar_op + l_read_name + ceil(l_seq / 2) + l_seq <= block_size - 32
ROCCO_BAM_FN bool bam_plausible_header(const uint8_t *b, long long o, int n_ref)
{
    const long long block_size = bam_i32(b, o);
    const int ref = bam_i32(b, o + 4), next_ref = bam_i32(b, o + 24);
    const long long l_read_name = bam_u8(b, o + 12), n_cigar = bam_u16(b, o + 16), l_seq = bam_i32(b, o + 20);
    return block_size >= kBamMinBlockSize && ref >= -1 && ref < n_ref && next_ref >= -1 && next_ref < n_ref && l_read_name >= 1 &&
           l_seq >= 0 && 4 * n_cigar + l_read_name + (l_seq + 1) / 2 + l_seq <= block_size - kBamMinBlockSize;
}

// kBamGuessDepth records in a row from offset o are plausible.  The first needs its 36 bytes inside the stream; a chain
// that runs off the stream's end behind it (a later header cut short, or a record that ends past n_bytes) is plausible --
// where it ends less than kBamRunoff bytes past n_bytes.  The bound is this project's: three bytes in front of a true
// record on contig 0 the four bytes of a "block_size" are the tail of the record before and the low byte of the true
// block_size, 16 MiB or more; the "refID" behind it is 0; and without a bound that chain leaves any slab at once and is
// accepted at depth 1 (the fixtures showed it: tests/golden/make_golden_bam_files.py).  A slab is cut at a BGZF block
// boundary and a block holds less than 64 KiB, so a record of ordinary length that the slab's end cuts ends within the bound.
// `head` is where the FIRST header is read from, as head + head_o (the guess kernel keeps a tile of the stream in LDS).
ROCCO_BAM_FN bool bam_plausible_chain(const uint8_t *bytes, long long n_bytes, long long o, int n_ref, const uint8_t *head,
                                      long long head_o)
{
    if (o < 0 || o + kBamFixed > n_bytes || !bam_plausible_header(head, head_o, n_ref)) {
        return false;
    }
    long long p = o + 4 + (long long)bam_i32(head, head_o);
    for (int k = 1; k < kBamGuessDepth; ++k) {
        if (p + kBamFixed > n_bytes) {
            return p - n_bytes < kBamRunoff;
        }
        if (!bam_plausible_header(bytes, p, n_ref)) {
            return false;
        }
        p += 4 + (long long)bam_i32(bytes, p);
    }
    return p - n_bytes < kBamRunoff;
}

// why a walk stopped (0: it reached its segment's end, or the stream's end exactly)
enum : int {
    kBamStopNone = 0,
    kBamStopBlockSize = ROCCO_BAM_ERR_BLOCK_SIZE,  // a block_size below 32
    kBamStopTruncated = ROCCO_BAM_ERR_TRUNCATED,   // the block_size word or the record it announces ends past n_bytes
};

// Walks the chain from p to the first offset >= seg_end (the exit, returned).  Counts the starts it passes, stores them at
// out[0 .. capacity) when Store.  Every load lies in [0, n_bytes).
template <bool Store>
ROCCO_BAM_FN long long bam_walk_segment(const uint8_t *bytes, long long n_bytes, long long p, long long seg_end, long long *out,
                                        long long capacity, long long *count_out, int *stop_out)
{
    long long count = 0;
    int stop = kBamStopNone;
    while (p < seg_end && p != n_bytes) {
        if (p + 4 > n_bytes) {
            stop = kBamStopTruncated;
            break;
        }
        const long long block_size = bam_i32(bytes, p);
        if (block_size < kBamMinBlockSize) {
            stop = kBamStopBlockSize;
            break;
        }
        if (p + 4 + block_size > n_bytes) {
            stop = kBamStopTruncated;
            break;
        }
        if (Store && count < capacity) {
            out[count] = p;
        }
        ++count;
        p += 4 + block_size;
    }
    *count_out = count;
    *stop_out = stop;
    return p;
}

}  // namespace

}  // namespace rocco
