// rocco_amd/csrc/fragments_rules.h -- the text of a fragments file (contig<TAB>start<TAB>end<TAB>barcode<TAB>count lines) ->
// per line (start, end, weight, name index, status word), and those -> bins: the rules, written ONCE for the kernels of
// fragments_file.hip, for their host twin and for tests/tools/fragments_rules_san.cpp (note (34)).
//
// What the reference's ccounts_sourceKindFragments branches do with a line once htslib has handed it over
// (rocco/native/ccounts_backend.c: 359-394 the strict integer parser, 311-357 the barcode lookup, 2212-2346 the region
// count, 1583-1631 the chromosome range, 1770-1835 the mapped count, 712-772 the read length).  A field ends at '\t', at the
// end of the line, at '\r' or at NUL; this project refuses a line with a NUL or with a '\r' that does not stand directly
// before its '\n', so a field here ends at '\t' or at the end of the content.  The four consumers scan different numbers of
// fields and stop at different places; `fragline_parse` records what each of them needs in one pass and the four
// predicates below read it from the status word.
//
// Everything here is bounded by what the caller states: a line is [at, at + length) and no byte outside it is read; a name
// or an allow-list entry is [offsets[i], offsets[i + 1]) of its packed bytes.  Plain C++ besides the __host__ __device__ marks.
#pragma once

#include <stdint.h>

#include "../../include/rocco_hip.h"

#if defined(__HIPCC__)
#define ROCCO_FRAGRULES_HD __host__ __device__ inline
#else
#define ROCCO_FRAGRULES_HD inline
#endif

namespace rocco {

constexpr long long kFragLimit = 1LL << 31;  // starts, ends and weights are kept in int32
constexpr int kFragCountDigits = 18;         // more digits than these in column 5 wrap the reference's int64

struct FragLine {
    int32_t start, end, weight, name;
    uint32_t status;
    int error;  // the lowest ROCCO_FRAGFILE_ERR_* the line earns, 0 for none
};

// a packed list of byte strings: entry i is bytes[offsets[i] .. offsets[i + 1])
struct FragNames {
    const uint8_t *bytes;
    const int64_t *offsets;
    long long first, last;  // the entries [first, last) are this caller's
};

// memcmp-like order of two byte strings, the shorter first where one is a prefix of the other (strcmp on strings without NUL)
ROCCO_FRAGRULES_HD int frag_compare(const uint8_t *a, long long na, const uint8_t *b, long long nb)
{
    const long long n = na < nb ? na : nb;
    for (long long i = 0; i < n; ++i) {
        if (a[i] != b[i]) {
            return a[i] < b[i] ? -1 : 1;
        }
    }
    return na == nb ? 0 : (na < nb ? -1 : 1);
}

// ccounts_barcodeAllowed (311-357) over a sorted list: true for an empty list
ROCCO_FRAGRULES_HD bool frag_allowed(const FragNames &list, const uint8_t *barcode, long long length)
{
    if (list.last <= list.first) {
        return true;
    }
    long long lo = list.first, hi = list.last - 1;
    while (lo <= hi) {
        const long long mid = lo + (hi - lo) / 2;
        const int cmp = frag_compare(list.bytes + list.offsets[mid], list.offsets[mid + 1] - list.offsets[mid], barcode, length);
        if (cmp == 0) {
            return true;
        }
        if (cmp < 0) {
            lo = mid + 1;
        } else {
            hi = mid - 1;
        }
    }
    return false;
}

// the index of the field among the entries [first, last) of a small list (ccounts_stringFieldInList: the first equal one), -1 for none
ROCCO_FRAGRULES_HD int frag_name_index(const FragNames &names, const uint8_t *field, long long length)
{
    for (long long i = names.first; i < names.last; ++i) {
        if (frag_compare(names.bytes + names.offsets[i], names.offsets[i + 1] - names.offsets[i], field, length) == 0) {
            return (int)i;
        }
    }
    return -1;
}

// ccounts_parseInt64Field (359-394) on a field: `ok` as the reference says it (an optional '-', then digits only; a lone
// '-' parses as 0; an empty field fails), `canonical` for "0" or [1-9][0-9]*, `digits` the number of digits.  The value
// saturates at 2^62 (the reference's would wrap beyond 18 digits; the callers refuse such a field before they use it).
struct FragInt {
    bool ok, canonical;
    int digits;
    long long value;
};

ROCCO_FRAGRULES_HD FragInt frag_parse_int(const uint8_t *field, long long length)
{
    FragInt r = {false, false, 0, 0};
    if (length <= 0) {
        return r;
    }
    long long i = field[0] == '-' ? 1 : 0;
    const bool negative = i == 1;
    long long value = 0;
    for (; i < length; ++i) {
        if (field[i] < '0' || field[i] > '9') {
            return r;
        }
        value = value < (1LL << 62) / 10 ? 10 * value + (field[i] - '0') : (1LL << 62);
        ++r.digits;
    }
    r.ok = true;
    r.canonical = !negative && r.digits > 0 && (field[0] != '0' || length == 1);
    r.value = negative ? -value : value;
    return r;
}

ROCCO_FRAGRULES_HD void frag_flag(FragLine *out, int code)
{
    if (out->error == 0 || code < out->error) {
        out->error = code;
    }
}

// One line, [at, at + length) with its terminator, of a span (whole_file == 0: the dialect of an index query; `names` holds
// the contigs a span may name) or of the whole file (whole_file != 0: hts_getline's lines, meta lines among them; `names`
// holds the contigs to leave out).  `allow` is the sorted allow-list of the line's track.
ROCCO_FRAGRULES_HD FragLine fragline_parse(const uint8_t *at, long long length, int whole_file, const FragNames &names, const FragNames &allow)
{
    FragLine out = {0, 0, 1, -1, 0u, 0};
    if (length > 0 && at[length - 1] == '\n') {  // (an unterminated last line is a line)
        --length;
        if (length > 0 && at[length - 1] == '\r') {
            --length;
        }
    }
    const bool meta = length > 0 && at[0] == '#';
    if (meta) {
        out.status |= ROCCO_FRAGFILE_META;
        if (!whole_file) {
            return out;  // (the index iterator skips the line)
        }
    }
    long long cursor = 0;
    int scanned = 0;              // fields the count rule's loop scans (all of them)
    bool last_empty = false;      // ... and whether the last of them is empty
    bool fifth_empty = true;      // the mapped rule's loop scans exactly five, past the end of the line if need be
    while (cursor < length) {
        const long long begin = cursor;
        while (cursor < length && at[cursor] != '\t') {
            if (at[cursor] == 0) {
                frag_flag(&out, ROCCO_FRAGFILE_ERR_NUL);
            } else if (at[cursor] == '\r') {
                frag_flag(&out, ROCCO_FRAGFILE_ERR_CR);
            }
            ++cursor;
        }
        const uint8_t *field = at + begin;
        const long long n = cursor - begin;
        if (scanned == 0) {
            out.name = frag_name_index(names, field, n);
        } else if (scanned == 1 || scanned == 2) {
            const FragInt v = frag_parse_int(field, n);
            // (tabix reads such a field with strtoll: another number; a meta line it never reads; an empty column of a whole
            // file's line is a column the line does not have)
            if (!v.canonical && !meta && !(whole_file && n == 0)) {
                out.status |= ROCCO_FRAGFILE_NONCANONICAL;
                frag_flag(&out, ROCCO_FRAGFILE_ERR_NONCANONICAL);
            }
            if (v.ok && (v.value >= kFragLimit || v.value <= -kFragLimit)) {
                out.status |= ROCCO_FRAGFILE_BEYOND;
                frag_flag(&out, ROCCO_FRAGFILE_ERR_BEYOND);
            } else if (v.ok) {
                (scanned == 1 ? out.start : out.end) = (int32_t)v.value;
                out.status |= scanned == 1 ? ROCCO_FRAGFILE_START_OK : ROCCO_FRAGFILE_END_OK;
            }
        } else if (scanned == 3) {
            if (n > 0) {
                out.status |= ROCCO_FRAGFILE_BARCODE_PRESENT;
            }
            if (n == 0 || frag_allowed(allow, field, n)) {
                out.status |= ROCCO_FRAGFILE_BARCODE_ALLOWED;
            }
        } else if (scanned == 4) {
            fifth_empty = n == 0;
            const FragInt v = frag_parse_int(field, n);
            if (v.ok && (v.digits > kFragCountDigits || v.value >= kFragLimit)) {
                out.status |= ROCCO_FRAGFILE_BEYOND;
                frag_flag(&out, ROCCO_FRAGFILE_ERR_COUNT);
            } else if (v.ok) {
                out.status |= ROCCO_FRAGFILE_WEIGHT_PARSED;
                out.weight = v.value > 0 ? (int32_t)v.value : 1;
            }
        }
        last_empty = n == 0;
        if (scanned < 7) {
            ++scanned;  // (the status word keeps min(fields, 5); 7 is past every use)
        }
        if (cursor < length) {
            ++cursor;  // (the tab; a tab that ends the line leaves an empty field behind it that the count rule never scans)
        }
    }
    const int fields = scanned < 5 ? scanned : 5;
    out.status |= (uint32_t)fields << ROCCO_FRAGFILE_FIELDS_SHIFT;
    if (scanned <= 3) {
        out.status |= ROCCO_FRAGFILE_BARCODE_ALLOWED;  // (no barcode: nothing to filter)
    }
    if (last_empty || scanned == 0) {
        out.status |= ROCCO_FRAGFILE_LAST_EMPTY;
    }
    if (fifth_empty) {
        out.status |= ROCCO_FRAGFILE_FIFTH_EMPTY;
    }
    if (!whole_file && scanned < 3) {
        // (a span's line without three fields ends tabix's iterator; the whole-file probes read short lines as the reference does)
        out.error = ROCCO_FRAGFILE_ERR_FIELDS;
    }
    return out;
}

ROCCO_FRAGRULES_HD bool frag_span_ok(uint32_t status)
{
    return (status & ROCCO_FRAGFILE_START_OK) != 0 && (status & ROCCO_FRAGFILE_END_OK) != 0;
}

// ccounts_getChromRange (1583-1631) and ccounts_getReadLength (712-772): three fields scanned, both integers parse, end > start
ROCCO_FRAGRULES_HD bool frag_valid_range(uint32_t status, int32_t start, int32_t end)
{
    return (status & ROCCO_FRAGFILE_META) == 0 && frag_span_ok(status) && end > start;
}

ROCCO_FRAGRULES_HD bool frag_valid_read_length(uint32_t status, int32_t start, int32_t end)
{
    return frag_span_ok(status) && end > start;  // (hts_getline: a meta line is a line)
}

// ccounts_countRegion (2212-2269): besides, the last field scanned is not empty and the barcode passes
ROCCO_FRAGRULES_HD bool frag_valid_count(uint32_t status, int32_t start, int32_t end)
{
    return frag_valid_range(status, start, end) && (status & ROCCO_FRAGFILE_LAST_EMPTY) == 0 && (status & ROCCO_FRAGFILE_BARCODE_ALLOWED) != 0;
}

// ccounts_getMappedReadCount (1770-1835): column 1 not excluded, a fifth field that is not empty, the barcode passes
ROCCO_FRAGRULES_HD bool frag_valid_mapped(uint32_t status, int32_t name)
{
    return name < 0 && (status & ROCCO_FRAGFILE_FIFTH_EMPTY) == 0 && (status & ROCCO_FRAGFILE_BARCODE_ALLOWED) != 0;
}

ROCCO_FRAGRULES_HD long long frag_mapped_weight(int32_t weight, int mode, int one_read_per_bin)
{
    const bool cut = mode == ROCCO_FRAGFILE_MODE_CUTSITE || mode == ROCCO_FRAGFILE_MODE_FIVEPRIME;
    return (long long)weight * (cut && !one_read_per_bin ? 2 : 1);
}

// What a counted line adds (2271-2345): up to two cells, each with a sign.  plus[0 .. n_plus) receive +weight,
// minus (>= 0) receives -weight (the cell behind index1, at most n_bins: the buffers hold n_bins + 1 cells).
struct FragCells {
    long long plus[2], minus;
    int n_plus;
};

ROCCO_FRAGRULES_HD FragCells frag_cells(long long start, long long end, int mode, int one_read_per_bin, long long r_start, long long r_end,
                                        long long step, long long n_bins)
{
    FragCells c = {{0, 0}, -1, 0};
    if (mode == ROCCO_FRAGFILE_MODE_CENTER || one_read_per_bin) {
        const long long mid = (start + end) / 2;
        if (mid >= r_start && mid < r_end && (mid - r_start) / step < n_bins) {
            c.plus[c.n_plus++] = (mid - r_start) / step;
        }
        return c;
    }
    if (mode == ROCCO_FRAGFILE_MODE_CUTSITE || mode == ROCCO_FRAGFILE_MODE_FIVEPRIME) {
        const long long cuts[2] = {start, end - 1};
        for (int k = 0; k < 2; ++k) {
            if (cuts[k] >= r_start && cuts[k] < r_end && (cuts[k] - r_start) / step < n_bins) {
                c.plus[c.n_plus++] = (cuts[k] - r_start) / step;
            }
        }
        return c;
    }
    if (end <= r_start || start >= r_end) {
        return c;
    }
    const long long a = start < r_start ? r_start : start, b = end > r_end ? r_end : end;
    const long long index0 = (a - r_start) / step;
    long long index1 = (b - 1 - r_start) / step;
    if (index0 >= n_bins) {
        return c;
    }
    if (index1 >= n_bins) {
        index1 = n_bins - 1;
    }
    if (index0 > index1) {
        return c;
    }
    c.plus[c.n_plus++] = index0;
    c.minus = index1 + 1;
    return c;
}

// the track of line i: the k with first[k] <= i < first[k + 1] (first ascends, first[K] > i)
ROCCO_FRAGRULES_HD long long frag_track(const int64_t *first, long long K, long long i)
{
    long long lo = 0, hi = K;
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (first[mid] <= i) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// ---- the host twin: the line pass and the field pass over host memory, on the calling thread -------------------------

// the lines of [entry0, n_bytes): starts_out (where given) receives every line start and, behind them, n_bytes; returns
// false where `capacity` holds fewer than n_lines + 1.  report: n_lines, the offset behind the last '\n' (entry0 for none),
// whether the last line is unterminated, 0.
inline bool fragfile_lines_host(const uint8_t *bytes, size_t n_bytes, size_t entry0, int64_t *starts_out, size_t capacity, int64_t *report)
{
    long long n_lines = 0, cut = (long long)entry0;
    for (size_t p = entry0; p < n_bytes; ++p) {
        if (bytes[p] == '\n') {
            ++n_lines;
            cut = (long long)p + 1;
        }
    }
    const bool open = entry0 < n_bytes && bytes[n_bytes - 1] != '\n';
    n_lines += open ? 1 : 0;
    report[0] = n_lines;
    report[1] = cut;
    report[2] = open ? 1 : 0;
    report[3] = 0;
    if (starts_out == nullptr) {
        return true;
    }
    if (capacity < (size_t)n_lines + 1) {
        return false;
    }
    size_t at = 0;
    if (entry0 < n_bytes) {
        starts_out[at++] = (int64_t)entry0;
    }
    for (size_t p = entry0; p + 1 < n_bytes; ++p) {
        if (bytes[p] == '\n') {
            starts_out[at++] = (int64_t)p + 1;
        }
    }
    starts_out[at] = (int64_t)n_bytes;
    return true;
}

// whether a line's error stands for a span's line or for a line of the whole file
ROCCO_FRAGRULES_HD int frag_line_error(const FragLine &line, int whole_file, int expect)
{
    int error = line.error;
    if (!whole_file && (line.status & ROCCO_FRAGFILE_META) == 0 && expect >= 0 && line.name != expect &&
        (error == 0 || ROCCO_FRAGFILE_ERR_CONTIG < error)) {
        error = ROCCO_FRAGFILE_ERR_CONTIG;
    }
    return error;
}

inline void fragfile_fields_host(const uint8_t *bytes, const int64_t *starts, size_t n_lines, int whole_file, const int64_t *track_first,
                                 const int32_t *expect, size_t K, const FragNames &names, const uint8_t *allow_bytes, const int64_t *allow_offsets,
                                 const int64_t *allow_first, int32_t *start_out, int32_t *end_out, int32_t *weight_out, int32_t *name_out,
                                 uint32_t *status_out, int64_t *report)
{
    report[0] = -1;
    report[1] = report[2] = report[3] = 0;
    long long previous = -1, previous_track = -1;  // the start of the span's last line that is no meta line
    for (size_t i = 0; i < n_lines; ++i) {
        const long long k = frag_track(track_first, (long long)K, (long long)i);
        const FragNames allow = {allow_bytes, allow_offsets, allow_first[k], allow_first[k + 1]};
        const FragLine line = fragline_parse(bytes + starts[i], starts[i + 1] - starts[i], whole_file, names, allow);
        start_out[i] = line.start;
        end_out[i] = line.end;
        weight_out[i] = line.weight;
        name_out[i] = line.name;
        status_out[i] = line.status;
        int error = frag_line_error(line, whole_file, expect[k]);
        if (!whole_file && (line.status & ROCCO_FRAGFILE_META) == 0) {
            if (previous_track == k && frag_span_ok(line.status) && previous > line.start && (error == 0 || ROCCO_FRAGFILE_ERR_ORDER < error)) {
                error = ROCCO_FRAGFILE_ERR_ORDER;
            }
            if (frag_span_ok(line.status)) {
                previous = line.start;
                previous_track = k;
            }
        }
        if (error != 0 && report[0] < 0) {
            report[0] = (int64_t)i;
            report[1] = error;
        }
    }
}

// ---- the barcode census (note (35)): ccounts_getCellCount (1890-2046) -----------------------

// The field the loop at 1937-1975 finds in one line [at, at + length): fields are separated by '\t'; the scan of the line
// ends at '\n', '\r' or NUL wherever they stand (and at the end of the bytes: hts_getline's string ends there); the barcode is
// field 3, with or without a field behind it.  false where the scan ends before field 3 or field 3 is empty: the line
// contributes nothing.  A line that begins with '#' is a line like any other; no other column is parsed or checked.
ROCCO_FRAGRULES_HD bool frag_barcode_field(const uint8_t *at, long long length, long long *offset, long long *n)
{
    long long cursor = 0;
    int field = 0;
    while (cursor < length && at[cursor] != 0 && at[cursor] != '\n' && at[cursor] != '\r') {
        const long long begin = cursor;
        while (cursor < length && at[cursor] != 0 && at[cursor] != '\t' && at[cursor] != '\n' && at[cursor] != '\r') {
            ++cursor;
        }
        if (field == 3) {
            *offset = begin;
            *n = cursor - begin;
            return cursor > begin;
        }
        if (cursor < length && at[cursor] == '\t') {
            ++cursor;
        }
        ++field;
    }
    return false;
}

// a 64-bit hash of a byte string: FNV-1a over the bytes, then the finalizer of splitmix64 (the low bits choose the slot, the
// high bits the tag: both must mix).  The census is exact whatever this returns; it only decides how long the probes are.
ROCCO_FRAGRULES_HD uint64_t frag_hash64(const uint8_t *bytes, long long n)
{
    uint64_t h = 0xcbf29ce484222325ULL;
    for (long long i = 0; i < n; ++i) {
        h = (h ^ (uint64_t)bytes[i]) * 0x100000001b3ULL;
    }
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ULL;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebULL;
    h ^= h >> 31;
    return h;
}

// A slot of the census table: 0 for empty, otherwise bit 63 set, bits 39..62 a tag from the masked hash, bit 38 set where the
// payload is an arena entry (clear: a line of the current slab), bits 0..37 that index.
constexpr int kCensusIndexBits = 38;
constexpr uint64_t kCensusIndexMask = (1ULL << kCensusIndexBits) - 1;
constexpr uint64_t kCensusArenaBit = 1ULL << kCensusIndexBits;
constexpr uint64_t kCensusTagMask = ((1ULL << 24) - 1) << 39;
constexpr uint64_t kCensusTaken = 1ULL << 63;

ROCCO_FRAGRULES_HD uint64_t census_word(uint64_t masked_hash, bool arena, uint64_t index)
{
    return kCensusTaken | ((masked_hash >> 1) & kCensusTagMask) | (arena ? kCensusArenaBit : 0) | (index & kCensusIndexMask);
}

ROCCO_FRAGRULES_HD uint64_t census_first_slot(uint64_t masked_hash, uint64_t capacity) { return masked_hash & (capacity - 1); }

// the smallest power of two that is at least 2 * wanted and at least ROCCO_BARCODE_CENSUS_MIN_CAPACITY
inline uint64_t census_capacity_for(uint64_t wanted)
{
    uint64_t capacity = ROCCO_BARCODE_CENSUS_MIN_CAPACITY;
    while (capacity < 2 * wanted) {
        capacity *= 2;
    }
    return capacity;
}

// The host twin: a plain sequential table under the same rule, hash, mask and growth bound, over all lines of `bytes` at
// once.  The entries come out in the order of their first line; `bytes_out` / `offsets_out` / `records_out` may be null for
// the sizes alone.  report: entries, the bytes of all barcodes, lines, grows.  false where an output is too small.
inline bool barcode_census_host(const uint8_t *bytes, size_t n_bytes, const FragNames &allow, uint64_t hash_mask, uint64_t initial_capacity,
                                uint8_t *bytes_out, size_t bytes_capacity, int64_t *offsets_out, int64_t *records_out, size_t entries_capacity,
                                int64_t *report)
{
    struct Entry {
        long long at, n;  // the barcode's bytes in `bytes`
        uint64_t hash;
        long long records;
    };
    uint64_t capacity = census_capacity_for(0);
    while (capacity < initial_capacity) {
        capacity *= 2;
    }
    // (index + 1 of the entry per slot, 0 for empty; grown by rehashing the stored hashes, as the device table is)
    size_t n_entries = 0, room = 64, total = 0;
    long long lines = 0, grows = 0;
    Entry *entries = new Entry[room];
    uint64_t *slots = new uint64_t[capacity]();
    size_t p = 0;
    while (p < n_bytes) {
        size_t end = p;
        while (end < n_bytes && bytes[end] != '\n') {
            ++end;
        }
        const long long length = (long long)(end < n_bytes ? end + 1 : end) - (long long)p;
        ++lines;
        long long offset = 0, n = 0;
        if (frag_barcode_field(bytes + p, length, &offset, &n) && frag_allowed(allow, bytes + p + offset, n)) {
            if (capacity < 2 * (n_entries + 1)) {
                const uint64_t grown = census_capacity_for(n_entries + 1);
                uint64_t *fresh = new uint64_t[grown]();
                for (size_t e = 0; e < n_entries; ++e) {
                    uint64_t slot = census_first_slot(entries[e].hash & hash_mask, grown);
                    while (fresh[slot] != 0) {
                        slot = (slot + 1) & (grown - 1);
                    }
                    fresh[slot] = e + 1;
                }
                delete[] slots;
                slots = fresh;
                capacity = grown;
                ++grows;
            }
            const uint64_t hash = frag_hash64(bytes + p + offset, n);
            uint64_t slot = census_first_slot(hash & hash_mask, capacity);
            while (slots[slot] != 0) {
                const Entry &e = entries[slots[slot] - 1];
                if (e.n == n && frag_compare(bytes + e.at, e.n, bytes + p + offset, n) == 0) {
                    break;
                }
                slot = (slot + 1) & (capacity - 1);
            }
            if (slots[slot] == 0) {
                if (n_entries == room) {
                    Entry *more = new Entry[2 * room];
                    for (size_t e = 0; e < n_entries; ++e) {
                        more[e] = entries[e];
                    }
                    delete[] entries;
                    entries = more;
                    room *= 2;
                }
                entries[n_entries] = {(long long)p + offset, n, hash, 0};
                slots[slot] = ++n_entries;
                total += (size_t)n;
            }
            ++entries[slots[slot] - 1].records;
        }
        p = end < n_bytes ? end + 1 : end;
    }
    report[0] = (int64_t)n_entries;
    report[1] = (int64_t)total;
    report[2] = lines;
    report[3] = grows;
    bool fits = true;
    if (offsets_out != nullptr || records_out != nullptr || bytes_out != nullptr) {
        fits = offsets_out != nullptr && (records_out != nullptr || n_entries == 0) && entries_capacity >= n_entries && bytes_capacity >= total &&
               (bytes_out != nullptr || total == 0);
        if (fits) {
            size_t to = 0;
            offsets_out[0] = 0;
            for (size_t e = 0; e < n_entries; ++e) {
                for (long long j = 0; j < entries[e].n; ++j) {
                    bytes_out[to++] = bytes[entries[e].at + j];
                }
                offsets_out[e + 1] = (int64_t)to;
                records_out[e] = entries[e].records;
            }
        }
    }
    delete[] entries;
    delete[] slots;
    return fits;
}

}  // namespace rocco
