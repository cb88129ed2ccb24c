// rocco_amd/csrc/barcode_census.hip -- the distinct barcodes of a fragments file and the lines of each, in HBM, gfx950
// (note (35)).  The rule of a line, the hash and the slot word are fragments_rules.h's, the same
// source the host twin compiles.
//
// insert: one lane per line over the starts of the line pass.  The lane finds its barcode, hashes it, ANDs the hash with the
//   caller's mask and probes an open-addressing table of 64-bit slots linearly from there.  On an empty slot it makes ONE
//   compare-and-swap with a word that names its own line; whatever the swap (or the atomic load before it) returns names
//   bytes that were written before the launch -- a line of this slab or an arena entry of an earlier one -- so the lane
//   compares bytes at once: equal, it adds 1 to the slot's counter; unequal, it probes the next slot.  No lane waits for
//   another and nothing is read through a plain load that another lane of the launch writes.  The host keeps
//   capacity >= 2 * (entries + lines of the slab), so a probe ends; a probe of `capacity` steps raises the error flag.
// settle: hipcub's exclusive sum over (1, length) of the lanes that won a swap gives every new representative its entry and
//   its place in the arena; one lane per representative copies the bytes, stores offset and hash and rewrites the slot to
//   arena form.  After it no slot names the slab.
// rehash: one lane per old slot places its entry in the new table by the stored hash (a swap on empty slots only: the
//   entries are distinct) and takes its counter along.  records: one lane per slot hands its counter to its entry.
// Counters are 64-bit integer atomics: the result does not depend on scheduling.  A barcode that holds most of a file's
// lines meets at one L2 atomic unit (DESIGN.md note (35)).
#include <hipcub/hipcub.hpp>

#include "fragments_rules.h"
#include "kernels.h"

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_FRAGFILE_THREADS;
constexpr int kLengthBits = kCensusIndexBits;  // the scan's word: the winners in the upper bits, their bytes in the lower 38
constexpr unsigned long long kLengthMask = (1ULL << kLengthBits) - 1;

struct CensusTable {
    unsigned long long *slots;
    long long *counts;
    unsigned long long capacity;  // a power of two
    const uint8_t *arena_bytes;
    const int64_t *arena_offsets;
    unsigned long long entries;
};

__device__ __forceinline__ unsigned long long slot_load(const unsigned long long *slot)
{
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 0 where this lane's word went into the empty slot, otherwise the word that stands there
__device__ __forceinline__ unsigned long long slot_claim(unsigned long long *slot, unsigned long long mine)
{
    unsigned long long expected = 0;
    __hip_atomic_compare_exchange_strong(slot, &expected, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;
}

// whether the bytes a taken slot's word names equal [barcode, barcode + n)
__device__ bool word_names(unsigned long long word, const CensusTable &table, const uint8_t *bytes, long long n_bytes, const int64_t *starts,
                           long long n_lines, const uint8_t *barcode, long long n)
{
    const unsigned long long index = word & kCensusIndexMask;
    const uint8_t *other = nullptr;
    long long other_n = 0;
    if ((word & kCensusArenaBit) != 0) {
        if (index >= table.entries) {
            return false;
        }
        other = table.arena_bytes + table.arena_offsets[index];
        other_n = table.arena_offsets[index + 1] - table.arena_offsets[index];
    } else {
        if (index >= (unsigned long long)n_lines) {
            return false;
        }
        const long long at = starts[index], next = starts[index + 1];
        long long offset = 0;
        if (at < 0 || at > next || next > n_bytes || !frag_barcode_field(bytes + at, next - at, &offset, &other_n)) {
            return false;
        }
        other = bytes + at + offset;
    }
    return other_n == n && frag_compare(other, other_n, barcode, n) == 0;
}

__global__ __launch_bounds__(kThreads) void census_insert_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, const int64_t *__restrict__ starts,
                                                                 long long n_lines, FragNames allow, CensusTable table, unsigned long long hash_mask,
                                                                 unsigned long long *__restrict__ won, unsigned long long *__restrict__ won_slot,
                                                                 unsigned long long *__restrict__ won_hash, unsigned int *__restrict__ overflow)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (long long)gridDim.x * kThreads) {
        unsigned long long mine_won = 0;
        const long long at = starts[i], next = starts[i + 1];
        long long offset = 0, n = 0;
        if (at >= 0 && at <= next && next <= n_bytes && frag_barcode_field(bytes + at, next - at, &offset, &n) &&
            frag_allowed(allow, bytes + at + offset, n)) {
            const uint8_t *barcode = bytes + at + offset;
            const unsigned long long hash = frag_hash64(barcode, n), masked = hash & hash_mask;
            const unsigned long long mine = census_word(masked, false, (unsigned long long)i);
            unsigned long long slot = census_first_slot(masked, table.capacity);
            bool placed = false;
            for (unsigned long long step = 0; step < table.capacity; ++step) {
                unsigned long long word = slot_load(table.slots + slot);
                if (word == 0) {
                    word = slot_claim(table.slots + slot, mine);
                    if (word == 0) {
                        mine_won = (1ULL << kLengthBits) | (unsigned long long)n;
                        won_slot[i] = slot;
                        won_hash[i] = hash;
                        placed = true;
                    }
                }
                if (!placed && ((word ^ mine) & kCensusTagMask) == 0 && word_names(word, table, bytes, n_bytes, starts, n_lines, barcode, n)) {
                    placed = true;
                }
                if (placed) {
                    __hip_atomic_fetch_add(table.counts + slot, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                slot = (slot + 1) & (table.capacity - 1);
            }
            if (!placed) {
                atomicOr(overflow, 1u);
            }
        }
        won[i] = mine_won;
    }
}

// won_first: the exclusive sum of the n_lines + 1 words of `won` (the last is 0)
__global__ __launch_bounds__(kThreads) void census_settle_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, const int64_t *__restrict__ starts,
                                                                 long long n_lines, const unsigned long long *__restrict__ won,
                                                                 const unsigned long long *__restrict__ won_first,
                                                                 const unsigned long long *__restrict__ won_slot,
                                                                 const unsigned long long *__restrict__ won_hash, unsigned long long *__restrict__ slots,
                                                                 unsigned long long capacity, uint8_t *__restrict__ arena_bytes,
                                                                 unsigned long long arena_bytes_capacity, int64_t *__restrict__ arena_offsets,
                                                                 unsigned long long *__restrict__ arena_hashes, unsigned long long arena_entries_capacity,
                                                                 unsigned long long entries, unsigned long long arena_used, unsigned long long hash_mask,
                                                                 unsigned int *__restrict__ overflow)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (long long)gridDim.x * kThreads) {
        if ((won[i] >> kLengthBits) == 0) {
            continue;
        }
        const unsigned long long entry = entries + (won_first[i] >> kLengthBits), to = arena_used + (won_first[i] & kLengthMask);
        const long long at = starts[i], next = starts[i + 1];
        long long offset = 0, n = 0;
        if (at < 0 || at > next || next > n_bytes || !frag_barcode_field(bytes + at, next - at, &offset, &n) || entry >= arena_entries_capacity ||
            to + (unsigned long long)n > arena_bytes_capacity || won_slot[i] >= capacity) {
            atomicOr(overflow, 2u);  // (the host's bounds rule this out)
            continue;
        }
        for (long long j = 0; j < n; ++j) {
            arena_bytes[to + j] = bytes[at + offset + j];
        }
        arena_offsets[entry + 1] = (int64_t)(to + (unsigned long long)n);
        arena_hashes[entry] = won_hash[i];
        __hip_atomic_store(slots + won_slot[i], census_word(won_hash[i] & hash_mask, true, entry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kThreads) void census_rehash_kernel(const unsigned long long *__restrict__ slots, const long long *__restrict__ counts,
                                                                 unsigned long long capacity, unsigned long long *__restrict__ new_slots,
                                                                 long long *__restrict__ new_counts, unsigned long long new_capacity,
                                                                 const unsigned long long *__restrict__ arena_hashes, unsigned long long entries,
                                                                 unsigned long long hash_mask, unsigned int *__restrict__ overflow)
{
    for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < capacity; s += (unsigned long long)gridDim.x * kThreads) {
        const unsigned long long word = slots[s];  // (written by earlier launches)
        if (word == 0) {
            continue;
        }
        const unsigned long long entry = word & kCensusIndexMask;
        if ((word & kCensusArenaBit) == 0 || entry >= entries) {
            atomicOr(overflow, 2u);  // (a slot that was not settled: not a table of this module)
            continue;
        }
        const unsigned long long masked = arena_hashes[entry] & hash_mask, mine = census_word(masked, true, entry);
        unsigned long long slot = census_first_slot(masked, new_capacity);
        bool placed = false;
        for (unsigned long long step = 0; step < new_capacity && !placed; ++step) {
            if (slot_load(new_slots + slot) == 0 && slot_claim(new_slots + slot, mine) == 0) {
                new_counts[slot] = counts[s];  // (no other lane has this slot)
                placed = true;
            } else {
                slot = (slot + 1) & (new_capacity - 1);
            }
        }
        if (!placed) {
            atomicOr(overflow, 1u);
        }
    }
}

__global__ __launch_bounds__(kThreads) void census_records_kernel(const unsigned long long *__restrict__ slots, const long long *__restrict__ counts,
                                                                  unsigned long long capacity, unsigned long long entries,
                                                                  long long *__restrict__ records, unsigned int *__restrict__ overflow)
{
    for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < capacity; s += (unsigned long long)gridDim.x * kThreads) {
        const unsigned long long word = slots[s];
        if (word == 0) {
            continue;
        }
        const unsigned long long entry = word & kCensusIndexMask;
        if ((word & kCensusArenaBit) == 0 || entry >= entries) {
            atomicOr(overflow, 2u);
            continue;
        }
        records[entry] = counts[s];
    }
}

unsigned census_grid(unsigned long long units)
{
    const unsigned long long groups = (units + kThreads - 1) / kThreads;
    return (unsigned)(groups < 1 ? 1 : (groups < ROCCO_BARCODE_CENSUS_MAX_GRID ? groups : ROCCO_BARCODE_CENSUS_MAX_GRID));
}

size_t won_scan_bytes(size_t n_lines)
{
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(n_lines + 1)) !=
        hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes > 0 ? bytes : 1;
}

// insert: per line the winner's word, its exclusive sum, its slot and its hash; the flag; hipcub's scan
struct InsertLayout {
    size_t won, won_first, won_slot, won_hash, overflow, scan, bytes;
    InsertLayout(size_t n_lines, size_t scan_bytes)
    {
        Layout lay;
        won = lay.at((n_lines + 1) * sizeof(unsigned long long));
        won_first = lay.at((n_lines + 1) * sizeof(unsigned long long));
        won_slot = lay.at((n_lines > 0 ? n_lines : 1) * sizeof(unsigned long long));
        won_hash = lay.at((n_lines > 0 ? n_lines : 1) * sizeof(unsigned long long));
        overflow = lay.at(sizeof(unsigned int));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

int overflow_status(unsigned int flag, const char *what)
{
    if (flag == 0) {
        return ROCCO_HIP_OK;
    }
    set_last_error(std::string(what) + ((flag & 1u) != 0 ? ": a probe went through the whole table without an empty slot or its barcode"
                                                          : ": a slot or an output index lies outside what the caller stated"));
    return ROCCO_HIP_EINVAL;
}

}  // namespace

size_t barcode_census_insert_scratch_bytes(size_t n_lines)
{
    const size_t scan = won_scan_bytes(n_lines);
    return scan == 0 ? 0 : InsertLayout(n_lines, scan).bytes;
}

int launch_barcode_census_insert(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines, const uint8_t *allow_bytes_dev,
                                 const int64_t *allow_offsets_dev, size_t n_allow, uint64_t *slots_dev, int64_t *counts_dev, size_t capacity,
                                 uint8_t *arena_bytes_dev, size_t arena_bytes_capacity, int64_t *arena_offsets_dev, uint64_t *arena_hashes_dev,
                                 size_t arena_entries_capacity, size_t entries, size_t arena_used, uint64_t hash_mask, int64_t *report_out_host,
                                 void *scratch_dev, hipStream_t stream)
{
    const InsertLayout at(n_lines, won_scan_bytes(n_lines));
    char *sc = (char *)scratch_dev;
    unsigned long long *won = (unsigned long long *)(sc + at.won), *won_first = (unsigned long long *)(sc + at.won_first);
    unsigned long long *won_slot = (unsigned long long *)(sc + at.won_slot), *won_hash = (unsigned long long *)(sc + at.won_hash);
    unsigned int *overflow = (unsigned int *)(sc + at.overflow), flag = 0;
    size_t scan_bytes = at.bytes - at.scan;
    unsigned long long total = 0;
    const CensusTable table = {(unsigned long long *)slots_dev, (long long *)counts_dev, (unsigned long long)capacity, arena_bytes_dev,
                               arena_offsets_dev, (unsigned long long)entries};
    const FragNames allow = {allow_bytes_dev, allow_offsets_dev, 0, (long long)n_allow};
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(unsigned int), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(won + n_lines, 0, sizeof(unsigned long long), stream));
        if (n_lines > 0) {
            hipLaunchKernelGGL(census_insert_kernel, dim3(census_grid(n_lines)), dim3(kThreads), 0, stream, bytes_dev, (long long)n_bytes, starts_dev,
                               (long long)n_lines, allow, table, (unsigned long long)hash_mask, won, won_slot, won_hash, overflow);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const unsigned long long *)won, won_first, (int)(n_lines + 1), stream));
        if (n_lines > 0) {
            hipLaunchKernelGGL(census_settle_kernel, dim3(census_grid(n_lines)), dim3(kThreads), 0, stream, bytes_dev, (long long)n_bytes, starts_dev,
                               (long long)n_lines, (const unsigned long long *)won, (const unsigned long long *)won_first,
                               (const unsigned long long *)won_slot, (const unsigned long long *)won_hash, (unsigned long long *)slots_dev,
                               (unsigned long long)capacity, arena_bytes_dev, (unsigned long long)arena_bytes_capacity, arena_offsets_dev,
                               (unsigned long long *)arena_hashes_dev, (unsigned long long)arena_entries_capacity, (unsigned long long)entries,
                               (unsigned long long)arena_used, (unsigned long long)hash_mask, overflow);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(&total, won_first + n_lines, sizeof(total), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(&flag, overflow, sizeof(flag), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the one wait: what the slab added, the flag; the slab may go)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    report_out_host[0] = (int64_t)(total >> kLengthBits);
    report_out_host[1] = (int64_t)(total & kLengthMask);
    report_out_host[2] = report_out_host[3] = 0;
    return overflow_status(flag, "barcode_census_insert");
}

int launch_barcode_census_rehash(const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity, uint64_t *new_slots_dev,
                                 int64_t *new_counts_dev, size_t new_capacity, const uint64_t *arena_hashes_dev, size_t entries, uint64_t hash_mask,
                                 void *scratch_dev, hipStream_t stream)
{
    unsigned int *overflow = (unsigned int *)scratch_dev, flag = 0;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(unsigned int), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(new_slots_dev, 0, new_capacity * sizeof(uint64_t), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(new_counts_dev, 0, new_capacity * sizeof(int64_t), stream));
        hipLaunchKernelGGL(census_rehash_kernel, dim3(census_grid(capacity)), dim3(kThreads), 0, stream, (const unsigned long long *)slots_dev,
                           (const long long *)counts_dev, (unsigned long long)capacity, (unsigned long long *)new_slots_dev,
                           (long long *)new_counts_dev, (unsigned long long)new_capacity, (const unsigned long long *)arena_hashes_dev,
                           (unsigned long long)entries, (unsigned long long)hash_mask, overflow);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(&flag, overflow, sizeof(flag), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the flag; the old table may go)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    return queued != ROCCO_HIP_OK ? queued : overflow_status(flag, "barcode_census_rehash");
}

int launch_barcode_census_records(const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity, size_t entries, int64_t *records_out_dev,
                                  void *scratch_dev, hipStream_t stream)
{
    unsigned int *overflow = (unsigned int *)scratch_dev, flag = 0;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(unsigned int), stream));
        hipLaunchKernelGGL(census_records_kernel, dim3(census_grid(capacity)), dim3(kThreads), 0, stream, (const unsigned long long *)slots_dev,
                           (const long long *)counts_dev, (unsigned long long)capacity, (unsigned long long)entries, (long long *)records_out_dev,
                           overflow);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(&flag, overflow, sizeof(flag), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    return queued != ROCCO_HIP_OK ? queued : overflow_status(flag, "barcode_census_records");
}

}  // namespace rocco
