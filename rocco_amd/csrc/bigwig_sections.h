// rocco_amd/csrc/bigwig_sections.h -- the inflated data sections of a bigWig file -> (start, end, value) intervals: the decode
// rules, written ONCE for the kernels of bigwig_sections.hip and for their host twin (note (31)).
//
// What libBigWig's bwGetOverlappingIntervals does with a data block once zlib has inflated it (bwValues.c: the 24-byte header
// `<IIIIIBBH` = chromId, chromStart, chromEnd, itemStep, itemSpan, type, reserved, itemCount; a block of another chromosome is
// left out; items of 12 / 8 / 4 bytes for bedGraph (1) / variableStep (2) / fixedStep (3); an item is kept unless
// end <= 0 || start >= the chromosome's length).  This project refuses what libBigWig would read past or wrap: a section
// shorter than its header or than its items, a type outside 1..3, an end beyond 2^32 - 1.
//
// Everything here is bounded by what the caller states: `section_fits` says whether a row of the block table and its
// `produced` lie inside the slots' buffer; `section_judge` reads the 24 header bytes only where produced >= 24 and accepts
// an item count only where 24 + count * size <= produced; an item is read at 24 + j * size + (0..size) with j < count.  The
// executor X says what a lane is: 64 lanes with ballots on the device, 1 lane on the host (as inflate_core.h does).  Plain
// C++ besides the __host__ __device__ marks: tests/tools/bigwig_sections_san.cpp compiles it under the host's sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/rocco_hip.h"

#if defined(__HIPCC__)
#define ROCCO_SECTIONS_HD __host__ __device__ inline
#else
#define ROCCO_SECTIONS_HD inline
#endif

namespace rocco {

constexpr long long kSectionHeaderBytes = 24;
constexpr long long kSectionMaxEnd = 0xFFFFFFFFLL;  // libBigWig keeps starts and ends in uint32_t

struct SectionHeader {
    long long chrom, start, step, span, count;
    int type, item_bytes;
};

// (a slot starts on a multiple of 8 by the host's stride, so items start on multiples of 4; nothing here relies on it)
ROCCO_SECTIONS_HD uint32_t section_u32(const uint8_t *at)
{
    uint32_t v;
    memcpy(&v, at, sizeof(v));
    return v;
}

// a row of the block table and the bytes its block inflated to, against the n_slots bytes they point into: the slot
// [offset, offset + capacity) lies in [0, n_slots) and 0 <= produced <= capacity
ROCCO_SECTIONS_HD bool section_fits(const int64_t *row, long long produced, long long n_slots)
{
    const long long capacity = row[2], offset = row[3];
    return capacity >= 0 && offset >= 0 && capacity <= n_slots && offset <= n_slots - capacity && produced >= 0 && produced <= capacity;
}

// the file of a block: the k with file_first[k] <= block < file_first[k + 1] (file_first ascends, file_first[n_files] > block)
ROCCO_SECTIONS_HD long long section_file(const long long *file_first, long long n_files, long long block)
{
    long long lo = 0, hi = n_files;  // (file_first[lo] <= block < file_first[hi])
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (file_first[mid] <= block) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// the header of a section of `produced` bytes: 0 and *skip = false (its items are to be read), 0 and *skip = true (it names
// another chromosome: nothing else of it is judged), or the ROCCO_BIGWIG_ERR_* that refuses it
ROCCO_SECTIONS_HD int section_judge(const uint8_t *sec, long long produced, long long want_chrom, SectionHeader *h, bool *skip)
{
    *skip = false;
    h->count = 0;
    if (produced < kSectionHeaderBytes) {
        return ROCCO_BIGWIG_ERR_SHORT;
    }
    h->chrom = section_u32(sec);
    h->start = section_u32(sec + 4);
    h->step = section_u32(sec + 12);
    h->span = section_u32(sec + 16);
    const uint32_t tail = section_u32(sec + 20);  // type, reserved, itemCount (little-endian)
    h->type = (int)(tail & 0xffu);
    if (h->chrom != want_chrom) {
        *skip = true;
        return 0;
    }
    if (h->type < 1 || h->type > 3) {
        return ROCCO_BIGWIG_ERR_TYPE;
    }
    h->item_bytes = h->type == 1 ? 12 : (h->type == 2 ? 8 : 4);
    const long long count = (long long)(tail >> 16);
    if (produced < kSectionHeaderBytes + count * h->item_bytes) {
        return ROCCO_BIGWIG_ERR_ITEMS;
    }
    h->count = count;
    return 0;
}

// item j (0 <= j < h.count) of a judged section, in 64-bit arithmetic.  Three loads at offsets the type decides, all inside
// the item (first word; the word behind it for bedGraph, else the first again; the last word, which is the value), and
// selects -- no branch on the type and no pointer that depends on one: hipcc -O3 of ROCm 7.2 turned the three-way branch
// with one load per arm (correct in its LLVM IR) into gfx950 code whose fixedStep arm loaded the value through a register
// pair that held j, not an address -- an illegal memory access on the first fixedStep section (DESIGN.md note (31)).
ROCCO_SECTIONS_HD void section_item(const uint8_t *sec, const SectionHeader &h, long long j, long long *start, long long *end, uint32_t *bits)
{
    const uint8_t *at = sec + kSectionHeaderBytes + j * h.item_bytes;
    const uint32_t first = section_u32(at), second = section_u32(at + (h.type == 1 ? 4 : 0));
    *bits = section_u32(at + (h.item_bytes - 4));
    *start = h.type == 3 ? h.start + j * h.step : (long long)first;
    *end = h.type == 1 ? (long long)second : *start + h.span;
}

ROCCO_SECTIONS_HD bool section_keeps(long long start, long long end, long long chrom_length)
{
    return !(end <= 0 || start >= chrom_length);
}

// the float32 of an item as the float64 that C's (double) makes of it on the reference's x86-64 (pyBigWig hands back
// PyFloat_FromDouble((double)value)): NaN payloads and the signs of zeros stay, a signalling NaN gets its quiet bit, a
// subnormal becomes a normal number.  Done on the bits, so that neither the denormal mode nor the NaN mode of a device has a say.
ROCCO_SECTIONS_HD uint64_t section_widen(uint32_t bits)
{
    const uint64_t sign = (uint64_t)(bits >> 31) << 63;
    const uint32_t exponent = (bits >> 23) & 0xffu;
    uint32_t fraction = bits & 0x7fffffu;
    if (exponent == 0xffu) {
        return sign | (0x7ffULL << 52) | ((uint64_t)fraction << 29) | (fraction != 0 ? 1ULL << 51 : 0ULL);
    }
    if (exponent != 0) {
        return sign | ((uint64_t)(exponent + 1023 - 127) << 52) | ((uint64_t)fraction << 29);
    }
    if (fraction == 0) {
        return sign;
    }
    int e = 1023 - 126;  // a subnormal float32 is a normal float64
    while ((fraction & 0x800000u) == 0) {
        fraction <<= 1;
        --e;
    }
    return sign | ((uint64_t)e << 52) | ((uint64_t)(fraction & 0x7fffffu) << 29);
}

// the executor of the host twin: one lane
struct HostSectionExec {
    static constexpr int kLanes = 1;
    int lane() const { return 0; }
    unsigned long long ballot(bool on) const { return on ? 1ULL : 0ULL; }
    static int bits(unsigned long long mask) { return (int)(mask & 1ULL); }
};

// the kept items of a judged section, and *wraps = true where one of its items ends beyond 2^32 - 1 (the section is then
// refused whole).  Every lane of X walks the turns together; all return the same values.
template <class X>
ROCCO_SECTIONS_HD long long section_count(const X &x, const uint8_t *sec, const SectionHeader &h, long long chrom_length, bool *wraps)
{
    long long kept = 0;
    bool wrapped = false;
    for (long long base = 0; base < h.count; base += X::kLanes) {
        const long long j = base + x.lane();
        bool keep = false, wrap = false;
        if (j < h.count) {
            long long start, end;
            uint32_t bits;
            section_item(sec, h, j, &start, &end, &bits);
            wrap = end > kSectionMaxEnd;
            keep = !wrap && section_keeps(start, end, chrom_length);
        }
        kept += X::bits(x.ballot(keep));
        wrapped = wrapped || x.ballot(wrap) != 0;
    }
    *wraps = wrapped;
    return kept;
}

// places the kept items of a judged section at [first, limit) of the three arrays, in item order; an index at or past
// `limit` is not written (limit is the least of the next block's first index and the arrays' capacity).  No LDS, no state
// that outlives a turn besides the running index.
template <class X>
ROCCO_SECTIONS_HD void section_emit(const X &x, const uint8_t *sec, const SectionHeader &h, long long chrom_length, long long first, long long limit,
                                    int64_t *starts, int64_t *ends, uint64_t *values)
{
    long long at = first;
    for (long long base = 0; base < h.count; base += X::kLanes) {
        const long long j = base + x.lane();
        bool keep = false;
        long long start = 0, end = 0;
        uint32_t bits = 0;
        if (j < h.count) {
            section_item(sec, h, j, &start, &end, &bits);
            keep = end <= kSectionMaxEnd && section_keeps(start, end, chrom_length);
        }
        const unsigned long long mask = x.ballot(keep);
        const unsigned long long below = x.lane() == 0 ? 0ULL : (mask & (~0ULL >> (64 - x.lane())));
        const long long to = at + X::bits(below);
        if (keep && to >= first && to < limit) {
            starts[to] = start;
            ends[to] = end;
            values[to] = section_widen(bits);
        }
        at += X::bits(mask);
    }
}

// the facts of block i: its status and its kept items (0 where it is refused or skipped).  Reads nothing of a row that does
// not fit.
template <class X>
ROCCO_SECTIONS_HD int section_facts(const X &x, const uint8_t *slots, long long n_slots, const int64_t *row, long long produced, long long want_chrom,
                                    long long chrom_length, long long *kept)
{
    *kept = 0;
    if (!section_fits(row, produced, n_slots)) {
        return ROCCO_BGZF_ERR_TABLE;
    }
    SectionHeader h;
    bool skip;
    const int judged = section_judge(slots + row[3], produced, want_chrom, &h, &skip);
    if (judged != 0 || skip) {
        return judged;
    }
    bool wraps;
    const long long n = section_count(x, slots + row[3], h, chrom_length, &wraps);
    if (wraps) {
        return ROCCO_BIGWIG_ERR_WRAP;
    }
    *kept = n;
    return 0;
}

// what the file arrays of a call must hold: file_first ascends from 0 to n_blocks
inline bool section_files_ok(const int64_t *file_first, size_t n_files, size_t n_blocks)
{
    if (file_first[0] != 0 || file_first[n_files] != (int64_t)n_blocks) {
        return false;
    }
    for (size_t k = 0; k < n_files; ++k) {
        if (file_first[k] > file_first[k + 1]) {
            return false;
        }
    }
    return true;
}

// The host twin, both stages over HOST memory on the calling thread.  Stage 1 (starts_out == nullptr): statuses, the
// n_blocks + 1 first indices, the n_files + 1 interval offsets, the report.  Stage 2 (starts_out given): stage 1, then the
// items, where no block is refused and the total fits `capacity`.  Returns false where the arguments are refused.
inline bool sections_host(const uint8_t *slots, size_t n_slots, const int64_t *table, const int64_t *produced, size_t n_blocks,
                          const int64_t *file_first, const int64_t *chrom_id, const int64_t *chrom_length, size_t n_files, int32_t *status_out,
                          int64_t *block_first_out, int64_t *file_offsets_out, int64_t *starts_out, int64_t *ends_out, uint64_t *values_out,
                          size_t capacity, int64_t *report_out)
{
    const HostSectionExec x;
    long long total = 0;
    report_out[0] = -1;
    report_out[1] = report_out[2] = report_out[3] = 0;
    size_t k = 0;
    for (size_t i = 0; i < n_blocks; ++i) {
        while (file_first[k + 1] <= (int64_t)i) {
            ++k;
        }
        long long kept = 0;
        const int status = section_facts(x, slots, (long long)n_slots, table + i * ROCCO_ZLIB_TABLE_COLUMNS, produced[i], chrom_id[k], chrom_length[k], &kept);
        status_out[i] = status;
        block_first_out[i] = total;
        total += kept;
        if (status != 0 && report_out[0] < 0) {
            report_out[0] = (int64_t)i;
            report_out[1] = status;
        }
    }
    block_first_out[n_blocks] = total;
    for (size_t f = 0; f <= n_files; ++f) {
        file_offsets_out[f] = block_first_out[file_first[f]];
    }
    report_out[2] = total;
    if (starts_out == nullptr || report_out[0] >= 0) {
        return true;
    }
    if ((size_t)total > capacity) {
        return false;
    }
    k = 0;
    for (size_t i = 0; i < n_blocks; ++i) {
        while (file_first[k + 1] <= (int64_t)i) {
            ++k;
        }
        if (block_first_out[i + 1] == block_first_out[i]) {
            continue;
        }
        const int64_t *row = table + i * ROCCO_ZLIB_TABLE_COLUMNS;
        SectionHeader h;
        bool skip;
        section_judge(slots + row[3], produced[i], chrom_id[k], &h, &skip);
        section_emit(x, slots + row[3], h, chrom_length[k], block_first_out[i], block_first_out[i + 1], starts_out, ends_out, values_out);
    }
    return true;
}

}  // namespace rocco
