// rocco_amd/csrc/interval_count.hip -- decoded alignment records -> one count per (interval, file) (DESIGN.md section 0
// row f6), gfx950.
//
// Replaces the counting half of the reference's post-hoc scoring:
//   count_alignment_intervals (rocco/_hts_counts.c:571-836): one ccounts_countRegion call per interval with
//                             region = [start, end), intervalSizeBP = end - start and a count buffer of one float
//   its callers raw_count_matrix (rocco/scores.py:250-341) and, at the null's options, the pysam count of get_ecdf
//   (rocco/scores.py:697-713)
// The per-record rule is record_cells of record_cells.h (the copy count.hip uses) with step = end - start, n_bins = 1 and
// the region taken per interval.
//
// F files x C contigs are T = F * C tracks of position-sorted records (track f * C + c), concatenated.  Three steps on
// the stream, no host synchronisation in between:
//   interval_track_facts_kernel  per track: the largest span L = max(max(end, pos + 1) - pos) and whether pos ascends
//   interval_bounds_kernel       per (interval, file): two bisections in the track's pos give the candidates [lo, hi) --
//                                first pos > start - L, first pos >= end -- and ceil((hi - lo) / UNIT) work units;
//                                hipcub's exclusive scan turns the unit counts into unit offsets (the total stays on the device)
//   interval_count_kernel        a fixed grid; a wavefront takes units in a grid stride, finds its pair by bisecting the unit
//                                offsets, its 64 lanes read consecutive records, record_cells, wave reduction, one integer
//                                atomicAdd (a plain store where the pair has one unit)
// Integer counts: the result does not depend on scheduling.  A long record widens L for its whole track: more candidates
// are read and filtered (time), never a wrong count.
//
// Row f12 (a contig group resident once, its peaks and null regions counted together): the same three steps with
// interval_sets_bounds_kernel / interval_sets_count_kernel -- every interval names one of up to four option sets, which
// travel by value in the kernel arguments, and the count of (interval p, file f) is stored at out[row[p] * out_stride +
// col0 + f]; the bounds kernel zeroes that cell, so exactly the addressed cells of out are written.
#include "kernels.h"
#include "record_cells.h"
#include "record_layouts.h"
#include "record_stream.h"

#include <hipcub/hipcub.hpp>

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_COUNT_INTERVALS_THREADS;
constexpr int kWave = 64;
constexpr int kWavesPerGroup = kThreads / kWave;
constexpr int kUnit = 256;                       // candidate records of one work unit
constexpr int kRecsPerLane = kUnit / kWave;
constexpr int kMaxGrid = ROCCO_COUNT_INTERVALS_MAX_GRID;  // workgroups of the counting launch
constexpr int kFactsMaxGrid = ROCCO_INTERVAL_FACTS_MAX_GRID;  // workgroups of interval_track_facts_kernel at most

static_assert(kUnit == ROCCO_COUNT_INTERVALS_UNIT && kWavesPerGroup == ROCCO_COUNT_INTERVALS_WAVES_PER_GROUP && kMaxGrid > 0 &&
                  kUnit % kWave == 0 && kThreads == 256 && kFactsMaxGrid > 0,
              "rocco_hip.h states the shape");

// facts[2 t]: L of track t; facts[2 t + 1]: 1 when some pos is smaller than the one before it
__global__ __launch_bounds__(kThreads) void interval_track_facts_kernel(const int *__restrict__ pos, const int *__restrict__ end,
                                                                       const long long *__restrict__ rec_offsets, int T,
                                                                       int *__restrict__ facts)
{
    const long long first = rec_offsets[0], total = rec_offsets[T];
    for (long long base = first + (long long)blockIdx.x * kThreads; base < total; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        int t = -1, span = 0, unsorted = 0;
        if (i < total) {
            t = find_slot(rec_offsets, T, i);
            const long long p = pos[i], e = end[i];
            span = (int)((e > p + 1 ? e : p + 1) - p);
            unsorted = (i > rec_offsets[t] && (long long)pos[i - 1] > p) ? 1 : 0;
        }
        const int t0 = __shfl(t, 0);
        if (__all(t == t0)) {  // (the usual case: a wavefront inside one track)
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const int s = __shfl_xor(span, off), u = __shfl_xor(unsorted, off);
                span = s > span ? s : span;
                unsorted |= u;
            }
            if ((threadIdx.x & (kWave - 1)) == 0 && t0 >= 0) {
                atomicMax(&facts[2 * t0], span);
                if (unsorted) {
                    atomicOr(&facts[2 * t0 + 1], 1);
                }
            }
        } else if (t >= 0) {
            atomicMax(&facts[2 * t], span);
            if (unsorted) {
                atomicOr(&facts[2 * t + 1], 1);
            }
        }
    }
}

// the candidates [*lo, *lo + *n) of region [s, e) on contig c of file f: first pos > s - L, first pos >= e; none for a
// contig outside [0, C) or an empty region
__device__ __forceinline__ void candidate_window(const int *__restrict__ pos, const long long *__restrict__ rec_offsets,
                                                 const int *__restrict__ facts, int f, int C, int c, long long s, long long e,
                                                 long long *lo, long long *n)
{
    if (c >= 0 && c < C && s >= 0 && e > s) {
        const int t = f * C + c;
        const long long b = rec_offsets[t], last = rec_offsets[t + 1];
        const long long L = facts[2 * t];
        *lo = lower_bound_pos(pos, b, last, s - L + 1);  // first pos > start - L
        const long long hi = lower_bound_pos(pos, *lo, last, e);  // first pos >= end (at or behind lo: start - L < end)
        *n = hi - *lo;
    }
}

// one thread per (interval p, file f), pair = p * F + f: cand_lo / cand_n = its candidates, units = its work units.
// units has pairs + 1 entries (the last one 0) so that the exclusive scan's last entry is the total.
__global__ __launch_bounds__(kThreads) void interval_bounds_kernel(const int *__restrict__ pos, const long long *__restrict__ rec_offsets,
                                                                  const int *__restrict__ facts, int F, int C,
                                                                  const int *__restrict__ contig_id, const int *__restrict__ start,
                                                                  const int *__restrict__ end, long long pairs,
                                                                  long long *__restrict__ cand_lo, int *__restrict__ cand_n,
                                                                  long long *__restrict__ units)
{
    const long long pair = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pair > pairs) {
        return;
    }
    if (pair == pairs) {
        units[pair] = 0;
        return;
    }
    const long long p = pair / F;
    const int f = (int)(pair - p * F);
    long long lo = 0, n = 0;
    candidate_window(pos, rec_offsets, facts, f, C, contig_id[p], start[p], end[p], &lo, &n);
    cand_lo[pair] = lo;
    cand_n[pair] = (int)n;
    units[pair] = (n + kUnit - 1) / kUnit;
}

__device__ __forceinline__ long long uniform64(long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the records [base, min(base + kUnit, limit)) that count for t's region (one bin), summed over the wavefront
__device__ __forceinline__ int count_unit(const CountTrack &t, const int *__restrict__ pos, const int *__restrict__ end,
                                          const int *__restrict__ isize, const unsigned short *__restrict__ flag,
                                          const unsigned char *__restrict__ mapq, const unsigned char *__restrict__ mate_same,
                                          long long base, long long limit, int lane)
{
    int count = 0;
#pragma unroll
    for (int j = 0; j < kRecsPerLane; ++j) {
        const long long r = base + j * kWave + lane;
        if (r < limit) {
            int i0 = -1, i1 = -1;
            if (record_cells(t, pos[r], end[r], isize[r], flag[r], mapq[r], mate_same[r], &i0, &i1)) {
                count += 1;  // (one bin: i0 == 0)
            }
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        count += __shfl_xor(count, off);
    }
    return count;
}

// unit_first: the exclusive scan of units (pairs + 1 entries; unit_first[pairs] is the number of units).  `options` holds
// the call's option set; its region fields are filled per interval.  out is zeroed before the launch.
__global__ __launch_bounds__(kThreads) void interval_count_kernel(
    const int *__restrict__ pos, const int *__restrict__ end, const int *__restrict__ isize,
    const unsigned short *__restrict__ flag, const unsigned char *__restrict__ mapq,
    const unsigned char *__restrict__ mate_same, CountTrack options, int F, const int *__restrict__ start,
    const int *__restrict__ stop, int pairs, const long long *__restrict__ cand_lo, const int *__restrict__ cand_n,
    const long long *__restrict__ unit_first, int *__restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long total_units = unit_first[pairs];
    const long long stride = (long long)gridDim.x * kWavesPerGroup;
    for (long long unit = uniform64((long long)blockIdx.x * kWavesPerGroup + (threadIdx.x / kWave)); unit < total_units; unit += stride) {
        const int pair = find_slot(unit_first, pairs, unit);
        const int p = pair / F;
        const long long first_unit = unit_first[pair];
        const long long lo = cand_lo[pair];
        const int n = cand_n[pair];
        CountTrack t = options;
        t.start = start[p];
        t.end = stop[p];
        t.step = t.end - t.start;  // intervalSizeBP = end - start (_hts_counts.c:571-836): one bin
        t.n_bins = 1;
        const int count = count_unit(t, pos, end, isize, flag, mapq, mate_same, lo + (unit - first_unit) * kUnit, lo + n, lane);
        if (lane == 0 && count != 0) {
            if (n <= kUnit) {
                out[pair] = count;  // the pair's only unit
            } else {
                atomicAdd(&out[pair], count);
            }
        }
    }
}

// ---- the same counting for a resident contig group with several option sets and placed output ----
// The S option sets of a call travel by value in the kernel arguments: a wavefront picks its interval's set once per unit.
struct CountSets {
    CountTrack set[ROCCO_COUNT_INTERVALS_MAX_SETS];
};

// where the counts of interval p go: out[row[p] * out_stride + col0 + f]
struct OutPlace {
    long long out_rows, out_stride, col0;
};

// interval_bounds_kernel for the sets call: an interval whose set id is outside [0, S) or whose row is outside
// [0, out_rows) raises *error and gets no unit and no store; every other pair's output cell is zeroed here, so that the
// count kernel adds into zeros and every cell nobody addresses keeps its contents.
__global__ __launch_bounds__(kThreads) void interval_sets_bounds_kernel(
    const int *__restrict__ pos, const long long *__restrict__ rec_offsets, const int *__restrict__ facts, int F, int C, int S,
    const int *__restrict__ set_id, const int *__restrict__ contig_id, const int *__restrict__ start, const int *__restrict__ end,
    const long long *__restrict__ row, OutPlace place, long long pairs, long long *__restrict__ cand_lo,
    int *__restrict__ cand_n, long long *__restrict__ units, int *__restrict__ out, int *__restrict__ error)
{
    const long long pair = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pair > pairs) {
        return;
    }
    if (pair == pairs) {
        units[pair] = 0;
        return;
    }
    const long long p = pair / F;
    const int f = (int)(pair - p * F);
    const int sid = set_id[p];
    const long long r = row[p];
    long long lo = 0, n = 0;
    if (sid < 0 || sid >= S || r < 0 || r >= place.out_rows) {
        if (f == 0) {
            atomicOr(error, 1);
        }
    } else {
        candidate_window(pos, rec_offsets, facts, f, C, contig_id[p], start[p], end[p], &lo, &n);
        out[r * place.out_stride + place.col0 + f] = 0;
    }
    cand_lo[pair] = lo;
    cand_n[pair] = (int)n;
    units[pair] = (n + kUnit - 1) / kUnit;
}

// interval_count_kernel with the option set and the output cell of the unit's interval.  Only pairs the bounds kernel
// accepted have units, so set_id[p] and row[p] are in range here.
__global__ __launch_bounds__(kThreads) void interval_sets_count_kernel(
    const int *__restrict__ pos, const int *__restrict__ end, const int *__restrict__ isize,
    const unsigned short *__restrict__ flag, const unsigned char *__restrict__ mapq,
    const unsigned char *__restrict__ mate_same, CountSets sets, int F, const int *__restrict__ set_id,
    const int *__restrict__ start, const int *__restrict__ stop, const long long *__restrict__ row, OutPlace place, int pairs,
    const long long *__restrict__ cand_lo, const int *__restrict__ cand_n, const long long *__restrict__ unit_first,
    int *__restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long total_units = unit_first[pairs];
    const long long stride = (long long)gridDim.x * kWavesPerGroup;
    for (long long unit = uniform64((long long)blockIdx.x * kWavesPerGroup + (threadIdx.x / kWave)); unit < total_units; unit += stride) {
        const int pair = __builtin_amdgcn_readfirstlane(find_slot(unit_first, pairs, unit));
        const int p = pair / F;
        const long long first_unit = unit_first[pair];
        const long long lo = cand_lo[pair];
        const int n = cand_n[pair];
        const int sid = __builtin_amdgcn_readfirstlane(set_id[p]);
        CountTrack t = sets.set[0];
#pragma unroll
        for (int s = 1; s < ROCCO_COUNT_INTERVALS_MAX_SETS; ++s) {
            if (sid == s) {
                t = sets.set[s];
            }
        }
        t.start = start[p];
        t.end = stop[p];
        t.step = t.end - t.start;  // intervalSizeBP = end - start (_hts_counts.c:571-836): one bin
        t.n_bins = 1;
        const int count = count_unit(t, pos, end, isize, flag, mapq, mate_same, lo + (unit - first_unit) * kUnit, lo + n, lane);
        if (lane == 0 && count != 0) {
            int *cell = out + (row[p] * place.out_stride + place.col0 + (pair - p * F));
            if (n <= kUnit) {
                *cell = count;  // the pair's only unit
            } else {
                atomicAdd(cell, count);
            }
        }
    }
}

// bytes hipcub's scan over the pairs + 1 unit counts wants
int size_interval_scan(size_t pairs, size_t &scan_bytes)
{
    scan_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const long long *)nullptr, (long long *)nullptr, (int)(pairs + 1)) !=
        hipSuccess) {
        (void)hipGetLastError();
        set_last_error("count_alignment_intervals: cannot size the scan");
        return ROCCO_HIP_EHIP;
    }
    return ROCCO_HIP_OK;
}

int check_interval_shape(const int64_t *rec_offsets_host, size_t F, size_t C, size_t P)
{
    if (F == 0 || C == 0 || P == 0 || F >= (1u << 20) || C >= (1u << 20) || F * C >= (size_t)0x7fffffff ||
        P >= (size_t)0x7fffffff || P * F >= (size_t)0x7ffffffe) {
        set_last_error("count_alignment_intervals: files x contigs or intervals x files is out of range");
        return ROCCO_HIP_EINVAL;
    }
    return check_record_tracks(rec_offsets_host, F * C, "count_alignment_intervals");
}

}  // namespace

size_t count_intervals_scratch_bytes(const int64_t *rec_offsets_host, size_t F, size_t C, size_t P)
{
    size_t scan_bytes = 0;
    if (check_interval_shape(rec_offsets_host, F, C, P) != ROCCO_HIP_OK || size_interval_scan(P * F, scan_bytes) != ROCCO_HIP_OK) {
        return 0;
    }
    return IntervalLayout(F * C, P * F, scan_bytes).bytes;
}

int launch_count_alignment_intervals(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                     const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                     const int64_t *rec_offsets_host, size_t F, size_t C, const rocco_hip_count_options *options_host,
                                     const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev, size_t P,
                                     int32_t *out_dev, int32_t *track_facts_out_host, void *scratch_dev, hipStream_t stream)
{
    const size_t T = F * C, pairs = P * F;
    size_t scan_bytes = 0;
    int rc = check_interval_shape(rec_offsets_host, F, C, P);
    if (rc != ROCCO_HIP_OK || (rc = size_interval_scan(pairs, scan_bytes)) != ROCCO_HIP_OK) {
        return rc;
    }
    const IntervalLayout at(T, pairs, scan_bytes);
    const CountTrack options = count_track_from_options(*options_host);
    std::vector<long long> offsets(rec_offsets_host, rec_offsets_host + T + 1);
    std::vector<int> facts(2 * T, 0);
    const long long records = offsets[T] - offsets[0];
    // the copies below read this call's host vectors: no return before the stream has taken them
    const int queued = queue_then_drain(stream, [&]() -> int {
        char *sc = (char *)scratch_dev;
        long long *rec_offsets = (long long *)(sc + at.rec_offsets), *cand_lo = (long long *)(sc + at.cand_lo);
        long long *units = (long long *)(sc + at.units), *unit_first = (long long *)(sc + at.unit_first);
        int *facts_dev = (int *)(sc + at.facts), *cand_n = (int *)(sc + at.cand_n);
        ROCCO_HIP_TRY(hipMemcpyAsync(rec_offsets, offsets.data(), (T + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(facts_dev, 0, 2 * T * sizeof(int), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(out_dev, 0, pairs * sizeof(int), stream));
        if (records > 0) {
            const long long blocks = (records + kThreads - 1) / kThreads;
            hipLaunchKernelGGL(interval_track_facts_kernel, dim3((unsigned)(blocks < kFactsMaxGrid ? blocks : kFactsMaxGrid)), dim3(kThreads), 0, stream,
                               (const int *)pos_dev, (const int *)end_dev, rec_offsets, (int)T, facts_dev);
        }
        hipLaunchKernelGGL(interval_bounds_kernel, dim3((unsigned)((pairs + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           (const int *)pos_dev, rec_offsets, facts_dev, (int)F, (int)C, (const int *)contig_id_dev,
                           (const int *)start_dev, (const int *)end_region_dev, (long long)pairs, cand_lo, cand_n, units);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const long long *)units, unit_first,
                                                       (int)(pairs + 1), stream));
        if (records > 0) {
            // at least one wavefront per pair is the most the launch can use when every pair has one unit; pairs with many
            // units are reached by the grid stride
            const size_t wanted = (pairs + kWavesPerGroup - 1) / kWavesPerGroup;
            const size_t by_records = (size_t)((records + kUnit - 1) / kUnit + kWavesPerGroup - 1) / kWavesPerGroup;
            size_t grid = wanted > by_records ? wanted : by_records;
            grid = grid < (size_t)kMaxGrid ? grid : (size_t)kMaxGrid;
            hipLaunchKernelGGL(interval_count_kernel, dim3((unsigned)grid), dim3(kThreads), 0, stream, (const int *)pos_dev,
                               (const int *)end_dev, (const int *)isize_dev, (const unsigned short *)flag_dev,
                               (const unsigned char *)mapq_dev, (const unsigned char *)mate_same_dev, options, (int)F,
                               (const int *)start_dev, (const int *)end_region_dev, (int)pairs, cand_lo, cand_n, unit_first,
                               (int *)out_dev);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(facts.data(), facts_dev, 2 * T * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the scratch buffer is the solver's; the facts are the caller's guard
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t i = 0; i < 2 * T; ++i) {
        track_facts_out_host[i] = facts[i];
    }
    return ROCCO_HIP_OK;
}

size_t count_intervals_sets_scratch_bytes(const int64_t *rec_offsets_host, size_t F, size_t C, size_t P)
{
    size_t scan_bytes = 0;
    if (check_interval_shape(rec_offsets_host, F, C, P) != ROCCO_HIP_OK || size_interval_scan(P * F, scan_bytes) != ROCCO_HIP_OK) {
        return 0;
    }
    return IntervalSetsLayout(F * C, P * F, scan_bytes).bytes;
}

int launch_count_alignment_intervals_sets(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                          const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                          const int64_t *rec_offsets_host, size_t F, size_t C,
                                          const rocco_hip_count_options *options_host, size_t S, const int32_t *set_id_dev,
                                          const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev,
                                          const int64_t *row_dev, size_t P, int32_t *out_dev, size_t out_rows, size_t out_stride,
                                          size_t col0, int32_t *track_facts_out_host, void *scratch_dev, hipStream_t stream)
{
    const size_t T = F * C, pairs = P * F;
    size_t scan_bytes = 0;
    int rc = check_interval_shape(rec_offsets_host, F, C, P);
    if (rc != ROCCO_HIP_OK || (rc = size_interval_scan(pairs, scan_bytes)) != ROCCO_HIP_OK) {
        return rc;
    }
    if (S == 0 || S > (size_t)ROCCO_COUNT_INTERVALS_MAX_SETS || out_rows == 0 || out_rows >= ((size_t)1 << 40) ||
        out_stride >= ((size_t)1 << 20) || col0 > out_stride || F > out_stride - col0) {
        set_last_error("count_alignment_intervals_sets: the number of option sets or the output placement is out of range");
        return ROCCO_HIP_EINVAL;
    }
    const IntervalSetsLayout at(T, pairs, scan_bytes);
    CountSets sets = {};
    for (size_t s = 0; s < S; ++s) {
        sets.set[s] = count_track_from_options(options_host[s]);
    }
    const OutPlace place = {(long long)out_rows, (long long)out_stride, (long long)col0};
    std::vector<long long> offsets(rec_offsets_host, rec_offsets_host + T + 1);
    std::vector<int> facts(2 * T + 1, 0);  // [2 T]: the error flag of the bounds kernel
    const long long records = offsets[T] - offsets[0];
    // the copies below read this call's host vectors: no return before the stream has taken them
    const int queued = queue_then_drain(stream, [&]() -> int {
        char *sc = (char *)scratch_dev;
        long long *rec_offsets = (long long *)(sc + at.rec_offsets), *cand_lo = (long long *)(sc + at.cand_lo);
        long long *units = (long long *)(sc + at.units), *unit_first = (long long *)(sc + at.unit_first);
        int *facts_dev = (int *)(sc + at.facts), *cand_n = (int *)(sc + at.cand_n);
        ROCCO_HIP_TRY(hipMemcpyAsync(rec_offsets, offsets.data(), (T + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(facts_dev, 0, (2 * T + 1) * sizeof(int), stream));
        if (records > 0) {
            const long long blocks = (records + kThreads - 1) / kThreads;
            hipLaunchKernelGGL(interval_track_facts_kernel, dim3((unsigned)(blocks < kFactsMaxGrid ? blocks : kFactsMaxGrid)), dim3(kThreads), 0, stream,
                               (const int *)pos_dev, (const int *)end_dev, rec_offsets, (int)T, facts_dev);
        }
        hipLaunchKernelGGL(interval_sets_bounds_kernel, dim3((unsigned)((pairs + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           (const int *)pos_dev, rec_offsets, facts_dev, (int)F, (int)C, (int)S, (const int *)set_id_dev,
                           (const int *)contig_id_dev, (const int *)start_dev, (const int *)end_region_dev,
                           (const long long *)row_dev, place, (long long)pairs, cand_lo, cand_n, units, (int *)out_dev,
                           facts_dev + 2 * T);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const long long *)units, unit_first,
                                                       (int)(pairs + 1), stream));
        if (records > 0) {
            // (the grid of launch_count_alignment_intervals)
            const size_t wanted = (pairs + kWavesPerGroup - 1) / kWavesPerGroup;
            const size_t by_records = (size_t)((records + kUnit - 1) / kUnit + kWavesPerGroup - 1) / kWavesPerGroup;
            size_t grid = wanted > by_records ? wanted : by_records;
            grid = grid < (size_t)kMaxGrid ? grid : (size_t)kMaxGrid;
            hipLaunchKernelGGL(interval_sets_count_kernel, dim3((unsigned)grid), dim3(kThreads), 0, stream, (const int *)pos_dev,
                               (const int *)end_dev, (const int *)isize_dev, (const unsigned short *)flag_dev,
                               (const unsigned char *)mapq_dev, (const unsigned char *)mate_same_dev, sets, (int)F,
                               (const int *)set_id_dev, (const int *)start_dev, (const int *)end_region_dev,
                               (const long long *)row_dev, place, (int)pairs, cand_lo, cand_n, unit_first, (int *)out_dev);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(facts.data(), facts_dev, (2 * T + 1) * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the call's one wait: the facts and the flag are the caller's guard
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t i = 0; i < 2 * T; ++i) {
        track_facts_out_host[i] = facts[i];
    }
    if (facts[2 * T] != 0) {
        set_last_error("count_alignment_intervals_sets: an interval's set id or output row is out of range");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

}  // namespace rocco
