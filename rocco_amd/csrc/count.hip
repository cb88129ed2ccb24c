// rocco_amd/csrc/count.hip -- decoded alignment records -> binned coverage, gfx950.
//
// Replaces what the reference does with a BAM record after htslib has decoded it:
//   ccounts_countRegion   (rocco/native/ccounts_backend.c:2400-2573, the alignment branch): filter, fragment, clip, difference
//                         array, running sum over the bins
//   ccounts_getChromRange (rocco/native/ccounts_backend.c:1666-1705): first start / last end of a contig
//   the tail of get_bam_chrom_reads (rocco/readtracks.py:492-517): scaling, positive support, np.round
// A record is six integers (pos, end = bam_endpos, isize, flag, mapq, mate on the same contig), in file order.
// For the K files of a chromosome at once (row f9): the ranges of all tracks in one launch, and the positive support of every
// track queued behind the counting (launch_track_supports); the matrix they lead to is written by track_matrix.hip.
//
// Counting is integer work: +1 / -1 into an int32 difference array with integer atomics (the result does not depend on
// scheduling), an int32 prefix sum, one conversion to float32.  The reference adds +-1.0f into float cells and runs a
// float sum: equal to the integers while every cell and every running value stays within +-2^24, which
// launch_count_alignment_records reports per track (the largest magnitude of a cell or a running value).
//
// Shape: position-sorted records put the 64 lanes of a wavefront on a few neighbouring bins, so a workgroup first
// aggregates its records in an LDS window of bins anchored at the lowest bin its records touch, and flushes the
// non-zero cells with one global atomic each; indices past the window (the far end of a long fragment) go to global
// memory directly.  The prefix sum is reduce-then-scan over tiles (three launches, no waiting between workgroups).
#include "count_tail.h"
#include "kernels.h"
#include "record_cells.h"
#include "record_layouts.h"
#include "record_stream.h"
#include "round_np.h"

#include <hipcub/hipcub.hpp>

#include <climits>

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_COUNT_THREADS;
constexpr int kRecsPerThread = 2;
constexpr int kRangeMaxGrid = ROCCO_CHROM_RANGE_MAX_GRID;  // workgroups of chrom_range_kernel at most
constexpr int kTailMaxGrid = ROCCO_COUNT_TAIL_MAX_GRID;    // workgroups of count_tail_kernel at most
constexpr int kMatrixMaxGrid = ROCCO_TRACK_MATRIX_MAX_GRID;  // workgroups of track_supports_kernel at most
constexpr int kChunk = kThreads * kRecsPerThread;  // records one workgroup aggregates at a time
constexpr int kWindow = 1024;                      // bins of the LDS window
constexpr int kScanItems = 8;
constexpr int kScanTile = kThreads * kScanItems;   // bins per scan tile

#ifdef ROCCO_COUNT_TOOL_MAX_GRID  // (tests/tools/alignment_count_bench.py tries other caps in its stand-alone builds)
constexpr int kMaxGrid = ROCCO_COUNT_TOOL_MAX_GRID;
#else
constexpr int kMaxGrid = ROCCO_COUNT_MAX_GRID;     // workgroups of one counting launch at most
#endif

static_assert(kChunk == ROCCO_COUNT_CHUNK_RECORDS && kScanTile == ROCCO_COUNT_SCAN_TILE && kWindow == ROCCO_COUNT_WINDOW_BINS &&
                  kMaxGrid > 0 && kThreads == 256 && kRangeMaxGrid > 0 && kTailMaxGrid > 0,
              "rocco_hip.h states the shape");

// chunk_first[k]: the first chunk of track k among all chunks (K + 1 entries).  A workgroup takes chunks blockIdx.x,
// blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kThreads) void count_records_kernel(
    const int *__restrict__ pos, const int *__restrict__ end, const int *__restrict__ isize,
    const unsigned short *__restrict__ flag, const unsigned char *__restrict__ mapq,
    const unsigned char *__restrict__ mate_same, const CountTrack *__restrict__ tracks, int K,
    const int *__restrict__ chunk_first, int total_chunks, int *__restrict__ delta)
{
    __shared__ int window[kWindow];
    __shared__ int s_anchor;
    for (int c = threadIdx.x; c < kWindow; c += kThreads) {
        window[c] = 0;
    }
    for (int chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
        const int k = find_slot(chunk_first, K, chunk);
        const CountTrack t = tracks[k];
        const long long base = t.rec_begin + (long long)(chunk - chunk_first[k]) * kChunk;
        int *__restrict__ track_delta = delta + t.delta_offset;
        if (threadIdx.x == 0) {
            s_anchor = INT_MAX;
        }
        __syncthreads();  // window zeroed (first pass or the last flush), anchor reset
        int i0[kRecsPerThread], i1[kRecsPerThread];
        int lowest = INT_MAX;
#pragma unroll
        for (int j = 0; j < kRecsPerThread; ++j) {
            const long long r = base + (long long)j * kThreads + threadIdx.x;
            i0[j] = -1;
            i1[j] = -1;
            if (r < t.rec_end) {
                int a = -1, b = -1;
                if (record_cells(t, pos[r], end[r], isize[r], flag[r], mapq[r], mate_same[r], &a, &b)) {
                    i0[j] = a;
                    i1[j] = b;
                    lowest = a < lowest ? a : lowest;  // (i1 > i0 always)
                }
            }
        }
#ifndef ROCCO_COUNT_NO_LDS_AGGREGATION
        lowest = wave_min(lowest);
        if ((threadIdx.x & (warpSize - 1)) == 0 && lowest != INT_MAX) {
            atomicMin(&s_anchor, lowest);
        }
        __syncthreads();
        const int anchor = s_anchor;
#pragma unroll
        for (int j = 0; j < kRecsPerThread; ++j) {
            if (i0[j] >= 0) {
                const unsigned off = (unsigned)(i0[j] - anchor);
                if (off < (unsigned)kWindow) {
                    atomicAdd(&window[off], 1);
                } else {
                    atomicAdd(&track_delta[i0[j]], 1);
                }
            }
            if (i1[j] >= 0) {
                const unsigned off = (unsigned)(i1[j] - anchor);
                if (off < (unsigned)kWindow) {
                    atomicSub(&window[off], 1);
                } else {
                    atomicSub(&track_delta[i1[j]], 1);
                }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < kWindow; c += kThreads) {
            const int v = window[c];
            if (v != 0) {  // (only cells some record of this chunk wrote: anchor + c <= n_bins)
                atomicAdd(&track_delta[(long long)anchor + c], v);
                window[c] = 0;
            }
        }
#else
#pragma unroll
        for (int j = 0; j < kRecsPerThread; ++j) {
            if (i0[j] >= 0) {
                atomicAdd(&track_delta[i0[j]], 1);
            }
            if (i1[j] >= 0) {
                atomicSub(&track_delta[i1[j]], 1);
            }
        }
#endif
    }
}

// ---- prefix sum over the bins: tile sums, their exclusive scan per track, scan + convert ---------------------------
__global__ __launch_bounds__(kThreads) void tile_sum_kernel(const CountTrack *__restrict__ tracks, int K,
                                                           const int *__restrict__ tile_first, const int *__restrict__ delta,
                                                           int *__restrict__ tile_sums)
{
    using Reduce = hipcub::BlockReduce<int, kThreads>;
    __shared__ typename Reduce::TempStorage temp;
    const int tile = blockIdx.x;
    const int k = find_slot(tile_first, K, tile);
    const long long base = (long long)(tile - tile_first[k]) * kScanTile;
    const int n_bins = tracks[k].n_bins;
    int sum = 0;
    if (!tracks[k].one_read_per_bin) {  // (those cells are the counts themselves: nothing runs across them)
        const int *__restrict__ cells = delta + tracks[k].delta_offset + base;
        for (int i = threadIdx.x; i < kScanTile && base + i < n_bins; i += kThreads) {
            sum += cells[i];
        }
    }
    sum = Reduce(temp).Sum(sum);
    if (threadIdx.x == 0) {
        tile_sums[tile] = sum;
    }
}

// one workgroup per track: tile_sums[first .. last) becomes its exclusive prefix sum
__global__ __launch_bounds__(kThreads) void tile_offsets_kernel(const int *__restrict__ tile_first, int *__restrict__ tile_sums)
{
    using Scan = hipcub::BlockScan<int, kThreads>;
    __shared__ typename Scan::TempStorage temp;
    const int first = tile_first[blockIdx.x], last = tile_first[blockIdx.x + 1];
    int carry = 0;
    for (int base = first; base < last; base += kThreads) {
        const int i = base + threadIdx.x;
        const int v = i < last ? tile_sums[i] : 0;
        int exclusive, total;
        Scan(temp).ExclusiveSum(v, exclusive, total);
        if (i < last) {
            tile_sums[i] = carry + exclusive;
        }
        carry += total;
        __syncthreads();  // temp is used again
    }
}

__global__ __launch_bounds__(kThreads) void scan_write_kernel(const CountTrack *__restrict__ tracks, int K,
                                                             const int *__restrict__ tile_first, const int *__restrict__ delta,
                                                             const int *__restrict__ tile_offsets, int accumulate,
                                                             float *__restrict__ out, int *__restrict__ max_magnitude)
{
    using Load = hipcub::BlockLoad<int, kThreads, kScanItems, hipcub::BLOCK_LOAD_WARP_TRANSPOSE>;
    using LoadF = hipcub::BlockLoad<float, kThreads, kScanItems, hipcub::BLOCK_LOAD_WARP_TRANSPOSE>;
    using Store = hipcub::BlockStore<float, kThreads, kScanItems, hipcub::BLOCK_STORE_WARP_TRANSPOSE>;
    using Scan = hipcub::BlockScan<int, kThreads>;
    using Reduce = hipcub::BlockReduce<int, kThreads>;
    __shared__ union {
        typename Load::TempStorage load;
        typename LoadF::TempStorage load_f;
        typename Store::TempStorage store;
        typename Scan::TempStorage scan;
        typename Reduce::TempStorage reduce;
    } temp;
    const int tile = blockIdx.x;
    const int k = find_slot(tile_first, K, tile);
    const long long base = (long long)(tile - tile_first[k]) * kScanTile;
    const int n_bins = tracks[k].n_bins;
    const int valid = (int)(n_bins - base < kScanTile ? n_bins - base : kScanTile);
    const int *__restrict__ cells = delta + tracks[k].delta_offset + base;
    float *__restrict__ track_out = out + tracks[k].out_offset + base;
    int v[kScanItems], run[kScanItems];
    Load(temp.load).Load(cells, v, valid, 0);
    __syncthreads();
    int biggest = 0;
    if (tracks[k].one_read_per_bin) {
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            run[i] = v[i];
        }
    } else {
        Scan(temp.scan).InclusiveSum(v, run);
        __syncthreads();
        const int offset = tile_offsets[tile];
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            run[i] += offset;
        }
        if (threadIdx.x == 0 && base + kScanTile >= n_bins) {
            const int past = cells[valid];  // the cell behind the last bin takes the -1 of every fragment that reaches it
            biggest = past < 0 ? -past : past;
        }
    }
    float f[kScanItems];
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        const int a = v[i] < 0 ? -v[i] : v[i], b = run[i] < 0 ? -run[i] : run[i];
        biggest = a > biggest ? a : biggest;
        biggest = b > biggest ? b : biggest;
        f[i] = (float)run[i];
    }
    if (accumulate) {  // countBuffer[i] += deltaValue (:2567): one float addition per bin
        float before[kScanItems];
        LoadF(temp.load_f).Load(track_out, before, valid, 0.0f);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            f[i] = before[i] + f[i];
        }
        if (tracks[k].one_read_per_bin) {
            // the reference adds 1.0f at a time into the used buffer (:2540): one addition gives the same float only while
            // the buffer holds integers and the sum stays within 2^24, so the sum counts towards the reported magnitude
#pragma unroll
            for (int i = 0; i < kScanItems; ++i) {
                const float m = fabsf(f[i]);
                const int mi = m < 2147483520.0f ? (int)m : INT_MAX;  // (NaN and infinity: INT_MAX)
                biggest = mi > biggest ? mi : biggest;
            }
        }
    }
    Store(temp.store).Store(track_out, f, valid);
    __syncthreads();
    biggest = Reduce(temp.reduce).Reduce(biggest, hipcub::Max());
    if (threadIdx.x == 0 && biggest > 0) {
        atomicMax(&max_magnitude[k], biggest);
    }
}

// ---- ccounts_getChromRange ------------------------------------------------------------------------------------------
// result[0]: lowest index of a record the first query yields and flag_exclude passes; result[1]: highest index + 1 of
// one the tail query yields and flag_exclude passes (0: none)
__global__ __launch_bounds__(kThreads) void chrom_range_kernel(const int *__restrict__ pos, const int *__restrict__ end,
                                                              const unsigned short *__restrict__ flag, long long n,
                                                              long long chrom_len, long long tail_start, int flag_exclude,
                                                              unsigned long long *__restrict__ result)
{
    unsigned long long first = ~0ULL, last = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        if ((flag[i] & flag_exclude) != 0) {
            continue;
        }
        const long long p = pos[i], e = end[i] > p + 1 ? end[i] : p + 1;
        if (p < chrom_len && e > 0) {  // sam_itr_queryi(0, chromLength), :1666
            first = (unsigned long long)i < first ? (unsigned long long)i : first;
        }
        if (p < chrom_len && e > tail_start) {  // sam_itr_queryi(tailStart, chromLength), :1686
            last = (unsigned long long)i + 1 > last ? (unsigned long long)i + 1 : last;
        }
    }
    wave_first_last(first, last, result);
}

__global__ void chrom_range_fetch_kernel(const int *__restrict__ pos, const int *__restrict__ end,
                                         const unsigned long long *__restrict__ result, long long *__restrict__ range)
{
    range[0] = result[0] != ~0ULL ? (long long)pos[result[0]] : 0;  // *startOut = record->core.pos (:1677)
    range[1] = result[1] != 0 ? (long long)end[result[1] - 1] : 0;  // *endOut = bam_endpos(record), the last one (:1701)
}

// ---- the tail of get_bam_chrom_reads (rocco/readtracks.py:492-517) ----------------------------------------------------
// vals = counts.astype(float64) * norm_scale; / float(step) if asked; * const_scale if const_scale >= 0; support[0] / [1]:
// first / last index + 1 with vals > 0 (before rounding); out = np.round(vals, digits)
__global__ __launch_bounds__(kThreads) void count_tail_kernel(const float *__restrict__ counts, long long n, double norm_scale,
                                                             int scale_by_step, double step, double const_scale, int apply_const,
                                                             double pow10, int digits, double *__restrict__ out,
                                                             unsigned long long *__restrict__ support)
{
    unsigned long long first = ~0ULL, last = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double v = count_tail_value(counts[i], norm_scale, scale_by_step, step, apply_const, const_scale);
        if (v > 0.0) {
            first = (unsigned long long)i < first ? (unsigned long long)i : first;
            last = (unsigned long long)i + 1;
        }
        out[i] = round_like_numpy(v, pow10, digits);
    }
    wave_first_last(first, last, support);
}

// ---- K tracks at once -------------------------------------------------------------------
// chrom_range_kernel for K tracks: a workgroup takes units of kThreads records of one track (unit_first: K + 1 ascending
// entries), in a grid stride.  first[k] / last[k] as result[0] / result[1] there, record indices into the concatenated arrays.
__global__ __launch_bounds__(kThreads) void chrom_range_batch_kernel(const int *__restrict__ pos, const int *__restrict__ end,
                                                                    const unsigned short *__restrict__ flag,
                                                                    const long long *__restrict__ rec_offsets,
                                                                    const long long *__restrict__ unit_first, int K, long long total_units,
                                                                    long long chrom_len, long long tail_start, int flag_exclude,
                                                                    unsigned long long *__restrict__ first_out,
                                                                    unsigned long long *__restrict__ last_out)
{
    for (long long unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
        const int k = find_slot(unit_first, K, unit);
        const long long i = rec_offsets[k] + (unit - unit_first[k]) * kThreads + threadIdx.x;
        unsigned long long first = ~0ULL, last = 0;
        if (i < rec_offsets[k + 1] && (flag[i] & flag_exclude) == 0) {
            const long long p = pos[i], e = end[i] > p + 1 ? end[i] : p + 1;
            if (p < chrom_len && e > 0) {
                first = (unsigned long long)i;
            }
            if (p < chrom_len && e > tail_start) {
                last = (unsigned long long)i + 1;
            }
        }
        wave_first_last(first, last, first_out + k, last_out + k);
    }
}

// range[2 k] = pos of track k's first record, range[2 k + 1] = end of its last one (0: none), as chrom_range_fetch_kernel
__global__ __launch_bounds__(kThreads) void chrom_range_batch_fetch_kernel(const int *__restrict__ pos, const int *__restrict__ end,
                                                                          const unsigned long long *__restrict__ first,
                                                                          const unsigned long long *__restrict__ last, int K,
                                                                          long long *__restrict__ range)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k < K) {
        range[2 * k] = first[k] != ~0ULL ? (long long)pos[first[k]] : 0;
        range[2 * k + 1] = last[k] != 0 ? (long long)end[last[k] - 1] : 0;
    }
}

// the support of count_tail_kernel for K tracks, without its values: first[k] / last[k] = lowest index / highest index + 1
// of a bin of track k whose scaled value is > 0.  A workgroup takes units of kSupportUnit bins of one track in a grid stride.
constexpr int kSupportPerThread = 4;
constexpr int kSupportUnit = kThreads * kSupportPerThread;

__global__ __launch_bounds__(kThreads) void track_supports_kernel(const float *__restrict__ counts, const SupportTrack *__restrict__ tracks,
                                                                 const long long *__restrict__ unit_first, int K, long long total_units,
                                                                 int scale_by_step, double step, double const_scale, int apply_const,
                                                                 unsigned long long *__restrict__ first_out,
                                                                 unsigned long long *__restrict__ last_out)
{
    for (long long unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
        const int k = find_slot(unit_first, K, unit);
        const SupportTrack t = tracks[k];
        const float *__restrict__ track_counts = counts + t.counts_offset;
        const long long base = (unit - unit_first[k]) * kSupportUnit;
        unsigned long long first = ~0ULL, last = 0;
#pragma unroll
        for (int j = 0; j < kSupportPerThread; ++j) {
            const long long i = base + (long long)j * kThreads + threadIdx.x;
            if (i < t.n_bins && count_tail_value(track_counts[i], t.norm_scale, scale_by_step, step, apply_const, const_scale) > 0.0) {
                first = (unsigned long long)i < first ? (unsigned long long)i : first;
                last = (unsigned long long)i + 1;
            }
        }
        wave_first_last(first, last, first_out + k, last_out + k);
    }
}

struct CountPlan {
    std::vector<CountTrack> tracks;
    std::vector<int> chunk_first, tile_first;
    CountLayout at = CountLayout(0, 0, 0);
};

int make_plan(const int64_t *rec_offsets, size_t K, const rocco_hip_count_options *options,
              const rocco_hip_count_region *regions, const int64_t *out_offsets, CountPlan &plan)
{
    const int rc = check_record_tracks(rec_offsets, K, "count_alignment_records");
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    plan.tracks.resize(K);
    plan.chunk_first.assign(K + 1, 0);
    plan.tile_first.assign(K + 1, 0);
    long long chunks = 0, tiles = 0;
    size_t cells = 0;
    for (size_t k = 0; k < K; ++k) {
        const rocco_hip_count_region &r = regions[k];
        if (r.step <= 0 || r.start < 0 || r.end <= r.start || r.n_bins <= 0 || out_offsets[k] < 0) {
            set_last_error("count_alignment_records: a track's region or output offset is invalid");
            return ROCCO_HIP_EINVAL;
        }
        CountTrack &t = plan.tracks[k];
        t = count_track_from_options(options[k]);
        t.rec_begin = rec_offsets[k];
        t.rec_end = rec_offsets[k + 1];
        t.out_offset = out_offsets[k];
        t.delta_offset = (long long)cells;
        t.start = r.start;
        t.end = r.end;
        t.step = r.step;
        t.n_bins = r.n_bins;
        plan.chunk_first[k] = (int)chunks;
        plan.tile_first[k] = (int)tiles;
        chunks += (t.rec_end - t.rec_begin + kChunk - 1) / kChunk;
        tiles += (long long)count_scan_tiles((size_t)r.n_bins);
        cells += count_delta_cells((size_t)r.n_bins);
        if (chunks >= INT_MAX || tiles >= INT_MAX) {
            set_last_error("count_alignment_records: too many records or bins for one call");
            return ROCCO_HIP_EINVAL;
        }
    }
    plan.chunk_first[K] = (int)chunks;
    plan.tile_first[K] = (int)tiles;
    plan.at = CountLayout(K, (size_t)tiles, cells);
    return ROCCO_HIP_OK;
}

// Queues the counting of `plan` on `stream` and waits for nothing: the caller keeps `plan` until the stream has taken its
// vectors, fetches *max_dev_out (K ints in the scratch buffer) and synchronises.
int queue_count(const CountPlan &plan, const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev, size_t K, int accumulate,
                float *out_dev, void *scratch_dev, hipStream_t stream, int **max_dev_out)
{
    char *sc = (char *)scratch_dev;
    CountTrack *tracks = (CountTrack *)(sc + plan.at.tracks);
    int *chunk_first = (int *)(sc + plan.at.chunk_first), *tile_first = (int *)(sc + plan.at.tile_first);
    int *max_dev = (int *)(sc + plan.at.maxima), *tile_sums = (int *)(sc + plan.at.tile_sums), *delta = (int *)(sc + plan.at.delta);
    ROCCO_HIP_TRY(hipMemcpyAsync(tracks, plan.tracks.data(), K * sizeof(CountTrack), hipMemcpyHostToDevice, stream));
    ROCCO_HIP_TRY(hipMemcpyAsync(chunk_first, plan.chunk_first.data(), (K + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
    ROCCO_HIP_TRY(hipMemcpyAsync(tile_first, plan.tile_first.data(), (K + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
    // the difference arrays and, in front of them, the per-track maxima and the tile sums: the tail of the layout
    ROCCO_HIP_TRY(hipMemsetAsync(max_dev, 0, plan.at.bytes - plan.at.maxima, stream));
    const int chunks = plan.chunk_first[K], tiles = plan.tile_first[K];
    if (chunks > 0) {
        const int grid = chunks < kMaxGrid ? chunks : kMaxGrid;
        hipLaunchKernelGGL(count_records_kernel, dim3((unsigned)grid), dim3(kThreads), 0, stream, (const int *)pos_dev,
                           (const int *)end_dev, (const int *)isize_dev, (const unsigned short *)flag_dev,
                           (const unsigned char *)mapq_dev, (const unsigned char *)mate_same_dev, tracks, (int)K, chunk_first,
                           chunks, delta);
    }
    hipLaunchKernelGGL(tile_sum_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, stream, tracks, (int)K, tile_first, delta,
                       tile_sums);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3((unsigned)K), dim3(kThreads), 0, stream, tile_first, tile_sums);
    hipLaunchKernelGGL(scan_write_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, stream, tracks, (int)K, tile_first, delta,
                       tile_sums, accumulate, out_dev, max_dev);
    ROCCO_HIP_TRY(hipGetLastError());
    *max_dev_out = max_dev;
    return ROCCO_HIP_OK;
}

}  // namespace

size_t count_alignment_scratch_bytes(const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                     const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host)
{
    CountPlan plan;
    if (make_plan(rec_offsets_host, K, options_host, regions_host, out_offsets_host, plan) != ROCCO_HIP_OK) {
        return 0;
    }
    return plan.at.bytes;
}

int launch_count_alignment_records(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                   const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                   const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                   const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                                   int accumulate, float *out_dev, int64_t *max_magnitude_out_host, void *scratch_dev,
                                   hipStream_t stream)
{
    CountPlan plan;
    const int rc = make_plan(rec_offsets_host, K, options_host, regions_host, out_offsets_host, plan);
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    std::vector<int> maxima(K, 0);
    // the copies below read this call's host vectors (plan's going up, `maxima` coming back): no return before the stream has
    // taken them
    const int queued = queue_then_drain(stream, [&]() -> int {
        int *max_dev = nullptr;
        if (const int q = queue_count(plan, pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, K, accumulate, out_dev,
                                      scratch_dev, stream, &max_dev);
            q != ROCCO_HIP_OK) {
            return q;
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(maxima.data(), max_dev, K * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the scratch buffer is the solver's; the maxima are the caller's guard
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t k = 0; k < K; ++k) {
        max_magnitude_out_host[k] = maxima[k];
    }
    return ROCCO_HIP_OK;
}

size_t track_supports_scratch_bytes(const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                    const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host)
{
    const size_t counting = count_alignment_scratch_bytes(rec_offsets_host, K, options_host, regions_host, out_offsets_host);
    return counting == 0 ? 0 : counting + SupportsLayout(K).bytes;
}

int launch_track_supports(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev, const uint16_t *flag_dev,
                          const uint8_t *mapq_dev, const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t K,
                          const rocco_hip_count_options *options_host, const rocco_hip_count_region *regions_host,
                          const int64_t *out_offsets_host, const double *norm_scale_host, int scale_by_step, double step,
                          double const_scale, float *out_dev, int64_t *max_magnitude_out_host, int64_t *support_out_host,
                          void *scratch_dev, hipStream_t stream)
{
    CountPlan plan;
    const int rc = make_plan(rec_offsets_host, K, options_host, regions_host, out_offsets_host, plan);
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    const SupportsLayout at(K);
    std::vector<SupportTrack> tracks(K);
    std::vector<long long> unit_first(K + 1, 0);
    for (size_t k = 0; k < K; ++k) {
        tracks[k] = SupportTrack{(long long)out_offsets_host[k], (long long)regions_host[k].n_bins, norm_scale_host[k]};
        unit_first[k + 1] = unit_first[k] + ((long long)regions_host[k].n_bins + kSupportUnit - 1) / kSupportUnit;
    }
    std::vector<int> maxima(K, 0);
    std::vector<unsigned long long> support(2 * K, 0);  // first[K] then last[K], as the layout keeps them
    const int queued = queue_then_drain(stream, [&]() -> int {
        int *max_dev = nullptr;
        if (const int q = queue_count(plan, pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, K, 0, out_dev, scratch_dev,
                                      stream, &max_dev);
            q != ROCCO_HIP_OK) {
            return q;
        }
        char *sc = (char *)scratch_dev + plan.at.bytes;  // behind the counter's regions
        SupportTrack *tracks_dev = (SupportTrack *)(sc + at.tracks);
        long long *unit_first_dev = (long long *)(sc + at.unit_first);
        unsigned long long *first_dev = (unsigned long long *)(sc + at.first), *last_dev = (unsigned long long *)(sc + at.last);
        ROCCO_HIP_TRY(hipMemcpyAsync(tracks_dev, tracks.data(), K * sizeof(SupportTrack), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(unit_first_dev, unit_first.data(), (K + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(first_dev, 0xff, K * sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(last_dev, 0, K * sizeof(unsigned long long), stream));
        const long long units = unit_first[K];
        hipLaunchKernelGGL(track_supports_kernel, dim3((unsigned)(units < (long long)kMatrixMaxGrid ? units : (long long)kMatrixMaxGrid)),
                           dim3(kThreads), 0, stream, (const float *)out_dev, tracks_dev, unit_first_dev, (int)K, units, scale_by_step,
                           step, const_scale, const_scale >= 0.0 ? 1 : 0, first_dev, last_dev);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(maxima.data(), max_dev, K * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(support.data(), first_dev, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(support.data() + K, last_dev, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the one wait of this call: the scratch buffer is the solver's
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t k = 0; k < K; ++k) {
        max_magnitude_out_host[k] = maxima[k];
        const bool any = support[K + k] != 0;
        support_out_host[2 * k] = any ? (int64_t)support[k] : -1;
        support_out_host[2 * k + 1] = any ? (int64_t)support[K + k] - 1 : -1;
    }
    return ROCCO_HIP_OK;
}

size_t chrom_range_batch_scratch_bytes(size_t K) { return RangeBatchLayout(K).bytes; }

int launch_alignment_chrom_range_batch(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev,
                                       const int64_t *rec_offsets_host, size_t K, int64_t chrom_len, int flag_exclude,
                                       int64_t *range_out_host, void *scratch_dev, hipStream_t stream)
{
    const int rc = check_record_tracks(rec_offsets_host, K, "alignment_chrom_range_batch");
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    for (size_t k = 0; k < 2 * K; ++k) {
        range_out_host[k] = 0;
    }
    const RangeBatchLayout at(K);
    std::vector<long long> rec_offsets(rec_offsets_host, rec_offsets_host + K + 1), unit_first(K + 1, 0);
    for (size_t k = 0; k < K; ++k) {
        unit_first[k + 1] = unit_first[k] + (rec_offsets[k + 1] - rec_offsets[k] + kThreads - 1) / kThreads;
    }
    const long long units = unit_first[K];
    if (units == 0) {
        return ROCCO_HIP_OK;
    }
    std::vector<long long> range(2 * K, 0);
    const int queued = queue_then_drain(stream, [&]() -> int {
        char *sc = (char *)scratch_dev;
        long long *rec_offsets_dev = (long long *)(sc + at.rec_offsets), *unit_first_dev = (long long *)(sc + at.unit_first);
        unsigned long long *first_dev = (unsigned long long *)(sc + at.first), *last_dev = (unsigned long long *)(sc + at.last);
        long long *range_dev = (long long *)(sc + at.range);
        ROCCO_HIP_TRY(hipMemcpyAsync(rec_offsets_dev, rec_offsets.data(), (K + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(unit_first_dev, unit_first.data(), (K + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(first_dev, 0xff, K * sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(last_dev, 0, K * sizeof(unsigned long long), stream));
        const long long tail_start = chrom_len > 2000000LL ? chrom_len - 2000000LL : 0;  // tailCushion (:1684)
        hipLaunchKernelGGL(chrom_range_batch_kernel, dim3((unsigned)(units < (long long)kRangeMaxGrid ? units : (long long)kRangeMaxGrid)),
                           dim3(kThreads), 0, stream, (const int *)pos_dev, (const int *)end_dev, (const unsigned short *)flag_dev,
                           rec_offsets_dev, unit_first_dev, (int)K, units, (long long)chrom_len, tail_start, flag_exclude, first_dev,
                           last_dev);
        hipLaunchKernelGGL(chrom_range_batch_fetch_kernel, dim3((unsigned)((K + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           (const int *)pos_dev, (const int *)end_dev, first_dev, last_dev, (int)K, range_dev);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(range.data(), range_dev, 2 * K * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the one wait of this call
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t k = 0; k < 2 * K; ++k) {
        range_out_host[k] = range[k];
    }
    return ROCCO_HIP_OK;
}

int launch_alignment_chrom_range(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev, size_t n,
                                 int64_t chrom_len, int flag_exclude, int64_t *start_out, int64_t *end_out, void *scratch_dev,
                                 hipStream_t stream)
{
    *start_out = 0;
    *end_out = 0;
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    unsigned long long *result = (unsigned long long *)scratch_dev;
    long long *range = (long long *)(result + 2);
    const unsigned long long init[2] = {~0ULL, 0ULL};
    ROCCO_HIP_TRY(hipMemcpyAsync(result, init, sizeof(init), hipMemcpyHostToDevice, stream));
    const long long tail_start = chrom_len > 2000000LL ? chrom_len - 2000000LL : 0;  // tailCushion (:1684)
    const size_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(chrom_range_kernel, dim3((unsigned)(blocks < (size_t)kRangeMaxGrid ? blocks : (size_t)kRangeMaxGrid)), dim3(kThreads), 0, stream,
                       (const int *)pos_dev, (const int *)end_dev, (const unsigned short *)flag_dev, (long long)n,
                       (long long)chrom_len, tail_start, flag_exclude, result);
    hipLaunchKernelGGL(chrom_range_fetch_kernel, dim3(1), dim3(1), 0, stream, (const int *)pos_dev, (const int *)end_dev, result,
                       range);
    ROCCO_HIP_TRY(hipGetLastError());
    long long host[2] = {0, 0};
    ROCCO_HIP_TRY(hipMemcpyAsync(host, range, sizeof(host), hipMemcpyDeviceToHost, stream));
    ROCCO_HIP_TRY(hipStreamSynchronize(stream));
    *start_out = host[0];
    *end_out = host[1];
    return ROCCO_HIP_OK;
}

int launch_alignment_count_tail(const float *counts_dev, size_t n, double norm_scale, int scale_by_step, double step,
                                double const_scale, int round_digits, double *vals_out_dev, int64_t *first_out,
                                int64_t *last_out, void *scratch_dev, hipStream_t stream)
{
    *first_out = -1;
    *last_out = -1;
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    unsigned long long *support = (unsigned long long *)scratch_dev;
    const unsigned long long init[2] = {~0ULL, 0ULL};
    ROCCO_HIP_TRY(hipMemcpyAsync(support, init, sizeof(init), hipMemcpyHostToDevice, stream));
    const size_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(count_tail_kernel, dim3((unsigned)(blocks < (size_t)kTailMaxGrid ? blocks : (size_t)kTailMaxGrid)), dim3(kThreads), 0, stream, counts_dev,
                       (long long)n, norm_scale, scale_by_step, step, const_scale, const_scale >= 0.0 ? 1 : 0,
                       numpy_pow10(round_digits), round_digits, vals_out_dev, support);
    ROCCO_HIP_TRY(hipGetLastError());
    unsigned long long host[2] = {~0ULL, 0ULL};
    ROCCO_HIP_TRY(hipMemcpyAsync(host, support, sizeof(host), hipMemcpyDeviceToHost, stream));
    ROCCO_HIP_TRY(hipStreamSynchronize(stream));
    if (host[1] != 0) {
        *first_out = (int64_t)host[0];
        *last_out = (int64_t)host[1] - 1;
    }
    return ROCCO_HIP_OK;
}

}  // namespace rocco

#ifdef ROCCO_COUNT_STANDALONE
// tests/tools/alignment_count_bench.py builds this file alone (once as it is, once with -DROCCO_COUNT_NO_LDS_AGGREGATION)
// to time the counting with and without the LDS window; the library itself never defines ROCCO_COUNT_STANDALONE.
namespace rocco {
void set_last_error(const std::string &msg) { fprintf(stderr, "count.hip: %s\n", msg.c_str()); }
}  // namespace rocco

extern "C" size_t rocco_count_standalone_scratch_bytes(const int64_t *rec_offsets, size_t K, const rocco_hip_count_options *options,
                                                       const rocco_hip_count_region *regions, const int64_t *out_offsets)
{
    return rocco::count_alignment_scratch_bytes(rec_offsets, K, options, regions, out_offsets);
}

extern "C" int rocco_count_standalone(const int32_t *pos, const int32_t *end, const int32_t *isize, const uint16_t *flag,
                                      const uint8_t *mapq, const uint8_t *mate_same, const int64_t *rec_offsets, size_t K,
                                      const rocco_hip_count_options *options, const rocco_hip_count_region *regions,
                                      const int64_t *out_offsets, float *out, int64_t *maxima, void *scratch, void *stream)
{
    return rocco::launch_count_alignment_records(pos, end, isize, flag, mapq, mate_same, rec_offsets, K, options, regions,
                                                 out_offsets, 0, out, maxima, scratch, (hipStream_t)stream);
}
#endif
