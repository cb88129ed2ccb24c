// rocco_amd/csrc/fragment_length.hip -- decoded alignment records of whole files -> the facts behind the reference's
// count metadata, gfx950.
//
// Replaces the record passes of
//   ccounts_getMappedReadCount (rocco/native/ccounts_backend.c:1712-1888)   record_flag_facts_kernel
//   ccounts_getFragmentLength  (rocco/native/ccounts_backend.c:861-1524):
//     1217-1311 chunk density and clamped window sums                       chunk_density_kernel, window_sums_kernel
//     1313      ranking by value descending, index ascending                hipcub's stable descending radix sort
//     1314-1339 greedy pick of block centres                                host C++ over a downloaded prefix of the ranking
//     1341-1469 strand cross-correlation of one block                       strand_xcorr_blocks_kernel
//     1084-1180 template lengths of the paired branch                       template_length_kernel + hipcub's stream compaction
// The sample pass (1015-1082) and the two head-of-file probes (598-856) look at a few thousand records: the caller does
// them on a downloaded head slice (rocco_amd/readtracks.py).
//
// Tracks are concatenated with T + 1 offsets, as in count.hip and interval_count.hip.  Everything a kernel adds up is an
// integer, except the lag scores: one lane per lag runs the reference's sum in the reference's order (sequential in i,
// multiply and add apart: -ffp-contract=off), so a score has the reference's bits on every schedule.
#include "kernels.h"
#include "record_layouts.h"
#include "record_stream.h"

#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_FRAGMENT_THREADS;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kDensityRecords = ROCCO_FRAGMENT_DENSITY_RECORDS;  // records a workgroup aggregates at a time
constexpr int kDensityWindow = ROCCO_FRAGMENT_DENSITY_WINDOW;    // cells of its LDS window
constexpr int kMaxBlockSize = ROCCO_FRAGMENT_MAX_BLOCK_SIZE;
constexpr int kMaxGrid = ROCCO_FRAGMENT_MAX_GRID;  // workgroups of a record pass at most

static_assert(kThreads == 256 && kDensityRecords % kThreads == 0 && kDensityWindow % kThreads == 0 && kMaxGrid > 0,
              "rocco_hip.h states the shape");
static_assert((size_t)kMaxBlockSize * 2 * sizeof(int) + 256 <= 160 * 1024, "two int32 arrays of a block fit one CU's LDS");

// mapped[t]: records of track t with flag & 4 == 0 (what hts_idx_get_stat reports as mapped for a contig);
// unsorted[t]: 1 when some pos is smaller than the one before it
__global__ __launch_bounds__(kThreads) void record_flag_facts_kernel(const int *__restrict__ pos, const unsigned short *__restrict__ flag,
                                                                    const long long *__restrict__ rec_offsets, int T,
                                                                    unsigned long long *__restrict__ mapped, int *__restrict__ unsorted)
{
    const long long first = rec_offsets[0], total = rec_offsets[T];
    for (long long base = first + (long long)blockIdx.x * kThreads; base < total; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        int t = -1, is_mapped = 0, bad = 0;
        if (i < total) {
            t = find_slot(rec_offsets, T, i);
            is_mapped = (flag[i] & 4) == 0 ? 1 : 0;
            bad = (i > rec_offsets[t] && pos[i - 1] > pos[i]) ? 1 : 0;
        }
        const int t0 = __shfl(t, 0);
        if (__all(t == t0)) {  // (the usual case: a wavefront inside one track)
            for (int off = kWave / 2; off > 0; off >>= 1) {
                is_mapped += __shfl_xor(is_mapped, off);
                bad |= __shfl_xor(bad, off);
            }
            if ((threadIdx.x & (kWave - 1)) == 0 && t0 >= 0) {
                if (is_mapped) {
                    atomicAdd(&mapped[t0], (unsigned long long)is_mapped);
                }
                if (bad) {
                    atomicOr(&unsorted[t0], 1);
                }
            }
        } else if (t >= 0) {
            if (is_mapped) {
                atomicAdd(&mapped[t], 1ULL);
            }
            if (bad) {
                atomicOr(&unsorted[t], 1);
            }
        }
    }
}

// ccounts_backend.c:1254-1269 for the records [lo, hi) of one track: raw[pos / chunk] += 1 for every record that passes
// flag_exclude and is not unmapped.  Records are position-sorted, so the kDensityRecords records of a workgroup's trip fall
// into a few neighbouring cells: they are counted in an LDS window that starts at the trip's first cell and flushed with one
// global atomic per touched cell; a cell outside the window (an unsorted track, a sparse one) is added to directly.
__global__ __launch_bounds__(kThreads) void chunk_density_kernel(const int *__restrict__ pos, const unsigned short *__restrict__ flag,
                                                                long long lo, long long hi, int flag_exclude, int chunk,
                                                                long long contig_len, int num_chunks, int *__restrict__ raw)
{
    __shared__ int window[kDensityWindow];
    for (long long base = lo + (long long)blockIdx.x * kDensityRecords; base < hi; base += (long long)gridDim.x * kDensityRecords) {
        for (int w = threadIdx.x; w < kDensityWindow; w += kThreads) {
            window[w] = 0;
        }
        const int first_cell = pos[base] / chunk;
        lds_barrier();
#pragma unroll
        for (int j = 0; j < kDensityRecords / kThreads; ++j) {
            const long long r = base + j * kThreads + threadIdx.x;
            if (r < hi) {
                const int f = flag[r];
                const int p = pos[r];
                if ((f & flag_exclude) == 0 && (f & 4) == 0 && p >= 0 && (long long)p < contig_len) {
                    const int cell = p / chunk;
                    if (cell < num_chunks) {
                        const int rel = cell - first_cell;
                        if (rel >= 0 && rel < kDensityWindow) {
                            atomicAdd(&window[rel], 1);
                        } else {
                            atomicAdd(&raw[cell], 1);
                        }
                    }
                }
            }
        }
        lds_barrier();
        for (int w = threadIdx.x; w < kDensityWindow; w += kThreads) {
            const int c = window[w];
            if (c != 0) {  // (only cells below num_chunks were counted)
                atomicAdd(&raw[first_cell + w], c);
            }
        }
        lds_barrier();
    }
}

// ccounts_backend.c:1274-1311: prefix[i] = raw[0] + .. + raw[i - 1] (num_chunks + 1 entries); the window of win_size
// cells around i, clamped at both ends of the contig by the reference's rules
__global__ __launch_bounds__(kThreads) void window_sums_kernel(const int *__restrict__ prefix, int num_chunks, int win_size,
                                                              int *__restrict__ density, int *__restrict__ index)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= num_chunks) {
        return;
    }
    long long start = i - win_size / 2;
    long long end = start + win_size;
    if (start < 0) {
        start = 0;
        end = win_size < num_chunks ? win_size : num_chunks;
    }
    if (end > num_chunks) {
        end = num_chunks;
        start = end - win_size;
        if (start < 0) {
            start = 0;
        }
    }
    density[i] = prefix[end] - prefix[start];
    index[i] = (int)i;
}

struct LagBest {
    double score;
    int lag;
};

// the larger score; the smaller lag where the scores compare equal (the reference's loop ascends in lag and replaces on a
// strict >); lag < 0: no lag seen
__device__ __forceinline__ LagBest better(LagBest a, LagBest b)
{
    if (a.lag < 0) {
        return b;
    }
    if (b.lag < 0) {
        return a;
    }
    if (b.score > a.score || (b.score == a.score && b.lag < a.lag)) {
        return b;
    }
    return a;
}

// ccounts_backend.c:1341-1469 for one block per workgroup.  Dynamic LDS: fwd[block_size], rev[block_size] as int32 counts;
// (double)count - mean, recomputed on use, is the double the reference stored.  A lane's loads do not depend on its
// accumulator: eight cells are loaded ahead of the eight dependent additions.  Lanes read rev at a stride of lag_step
// dwords: conflict-free on 32 banks for every odd lag_step (1, 5, 7), fwd[i] is one address for the whole wavefront.
__global__ __launch_bounds__(kThreads) void strand_xcorr_blocks_kernel(
    const int *__restrict__ pos, const int *__restrict__ end, const unsigned short *__restrict__ flag,
    const long long *__restrict__ rec_offsets, const int *__restrict__ block_track, const long long *__restrict__ block_start,
    const int *__restrict__ min_lag, int flag_exclude, int block_size, int max_insert, int lag_step, int *__restrict__ best_lag_out,
    double *__restrict__ best_score_out, int *__restrict__ fwd_sum_out, int *__restrict__ rev_sum_out)
{
    extern __shared__ int cells[];
    __shared__ int wave_fwd[kWaves], wave_rev[kWaves], wave_lag[kWaves];
    __shared__ double wave_score[kWaves];
    int *fwd = cells, *rev = cells + block_size;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int t = block_track[b];
    const long long start_bp = block_start[b], end_bp = start_bp + block_size;
    for (int i = tid; i < 2 * block_size; i += kThreads) {
        cells[i] = 0;
    }
    lds_barrier();
    const long long track_lo = rec_offsets[t], track_hi = rec_offsets[t + 1];
    const long long lo = lower_bound_pos(pos, track_lo, track_hi, start_bp);
    const long long hi = lower_bound_pos(pos, lo, track_hi, end_bp);
    for (long long r = lo + tid; r < hi; r += kThreads) {
        const int f = flag[r];
        const long long p = pos[r], e = end[r];
        if ((f & flag_exclude) != 0 || (f & 4) != 0 || e <= p || p < start_bp || e > end_bp) {
            continue;
        }
        if ((f & 16) == 0) {
            atomicAdd(&fwd[(int)(p - start_bp)], 1);  // (start_bp <= p < e <= end_bp)
        } else {
            atomicAdd(&rev[(int)(e - 1 - start_bp)], 1);
        }
    }
    lds_barrier();
    int fsum = 0, rsum = 0;
    for (int i = tid; i < block_size; i += kThreads) {
        fsum += fwd[i];
        rsum += rev[i];
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        fsum += __shfl_xor(fsum, off);
        rsum += __shfl_xor(rsum, off);
    }
    if (lane == 0) {
        wave_fwd[wave] = fsum;
        wave_rev[wave] = rsum;
    }
    lds_barrier();
    fsum = 0;
    rsum = 0;
    for (int w = 0; w < kWaves; ++w) {
        fsum += wave_fwd[w];
        rsum += wave_rev[w];
    }
    const int first_lag = min_lag[t];
    const int last_lag = max_insert < block_size - 1 ? max_insert : block_size - 1;
    const int n_lags = (fsum < 10 || rsum < 10 || last_lag < first_lag) ? 0 : (last_lag - first_lag) / lag_step + 1;
    const double fwd_mean = (double)fsum / (double)block_size, rev_mean = (double)rsum / (double)block_size;
    LagBest mine = {0.0, -1};
    for (int j = tid; j < n_lags; j += kThreads) {
        const int lag = first_lag + j * lag_step;
        const int len = block_size - lag;
        const int *shifted = rev + lag;
        double score = 0.0;
        int i = 0;
        for (; i + 8 <= len; i += 8) {
            int fc[8], rc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                fc[u] = fwd[i + u];
                rc[u] = shifted[i + u];
            }
            double product[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                product[u] = ((double)fc[u] - fwd_mean) * ((double)rc[u] - rev_mean);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                score += product[u];
            }
        }
        for (; i < len; ++i) {
            score += ((double)fwd[i] - fwd_mean) * ((double)shifted[i] - rev_mean);
        }
        const LagBest candidate = {score, lag};
        mine = better(mine, candidate);
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        LagBest other;
        other.score = __shfl_xor(mine.score, off);
        other.lag = __shfl_xor(mine.lag, off);
        mine = better(mine, other);
    }
    if (lane == 0) {
        wave_score[wave] = mine.score;
        wave_lag[wave] = mine.lag;
    }
    lds_barrier();
    if (tid == 0) {
        LagBest best = {0.0, -1};
        for (int w = 0; w < kWaves; ++w) {
            const LagBest other = {wave_score[w], wave_lag[w]};
            best = better(best, other);
        }
        best_lag_out[b] = best.lag;
        best_score_out[b] = best.lag < 0 ? 0.0 : best.score;
        fwd_sum_out[b] = fsum;
        rev_sum_out[b] = rsum;
    }
}

// ccounts_backend.c:1118-1143: |isize| of a record that qualifies as a template of the paired branch, -1 otherwise
__global__ __launch_bounds__(kThreads) void template_length_kernel(const int *__restrict__ isize, const unsigned short *__restrict__ flag,
                                                                  const unsigned char *__restrict__ mate_same,
                                                                  const long long *__restrict__ rec_offsets, int T,
                                                                  const int *__restrict__ min_insert, int flag_exclude, int max_insert,
                                                                  int *__restrict__ lengths)
{
    const long long first = rec_offsets[0], total = rec_offsets[T];
    for (long long i = first + (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const int f = flag[i];
        int value = -1;
        if ((f & flag_exclude) == 0 && (f & 2) != 0 && (f & 128) == 0 && (f & 8) == 0 && mate_same[i] != 0) {
            const long long length = isize[i] >= 0 ? (long long)isize[i] : -(long long)isize[i];
            if (length >= (long long)min_insert[find_slot(rec_offsets, T, i)] && length <= (long long)max_insert) {
                value = (int)length;
            }
        }
        lengths[i] = value;
    }
}

struct NotNegative {
    __host__ __device__ bool operator()(const int &v) const { return v >= 0; }
};

unsigned grid_for(long long items, int per_group)
{
    const long long groups = (items + per_group - 1) / per_group;
    return (unsigned)(groups < 1 ? 1 : (groups < kMaxGrid ? groups : kMaxGrid));
}

// number of chunks of a contig (ccounts_backend.c:1217), 0 where the reference skips the contig (1212-1221)
long long chunks_of(long long contig_len, int block_size, int chunk)
{
    if (contig_len < (long long)block_size) {
        return 0;
    }
    const long long n = (contig_len + chunk - 1) / chunk;
    return n < 1 ? 0 : n;
}

// bytes hipcub wants for the scan over max_chunks + 1 cells or the sort of max_chunks pairs, whichever is more
int size_centers_cub(long long max_chunks, size_t &cub_bytes)
{
    size_t scan_bytes = 0, sort_bytes = 0;
    const int n = (int)max_chunks;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const int *)nullptr, (int *)nullptr, n + 1) != hipSuccess ||
        hipcub::DeviceRadixSort::SortPairsDescending(nullptr, sort_bytes, (const int *)nullptr, (int *)nullptr, (const int *)nullptr,
                                                     (int *)nullptr, n) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("fragment_block_centers: cannot size the scan or the sort");
        return ROCCO_HIP_EHIP;
    }
    cub_bytes = scan_bytes > sort_bytes ? scan_bytes : sort_bytes;
    return ROCCO_HIP_OK;
}

long long max_chunks_of(const int64_t *contig_len_host, size_t T, int block_size, int chunk)
{
    long long most = 0;
    for (size_t t = 0; t < T; ++t) {
        const long long n = chunks_of(contig_len_host[t], block_size, chunk);
        most = n > most ? n : most;
    }
    return most;
}

}  // namespace

size_t record_flag_facts_scratch_bytes(size_t T) { return FlagFactsLayout(T).bytes; }

int launch_record_flag_facts(const int32_t *pos_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t T,
                             int64_t *mapped_out_host, int32_t *unsorted_out_host, void *scratch_dev, hipStream_t stream)
{
    int rc = check_record_tracks(rec_offsets_host, T, "record_flag_facts");
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    std::vector<long long> offsets(rec_offsets_host, rec_offsets_host + T + 1);
    std::vector<unsigned long long> mapped(T, 0);
    std::vector<int> unsorted(T, 0);
    const long long records = offsets[T] - offsets[0];
    const FlagFactsLayout at(T);
    char *sc = (char *)scratch_dev;
    long long *offsets_dev = (long long *)(sc + at.rec_offsets);
    unsigned long long *mapped_dev = (unsigned long long *)(sc + at.mapped);
    int *unsorted_dev = (int *)(sc + at.unsorted);
    // the copies below read and write this call's host vectors: no return before the stream is done with them
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemcpyAsync(offsets_dev, offsets.data(), (T + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(mapped_dev, 0, T * sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(unsorted_dev, 0, T * sizeof(int), stream));
        if (records > 0) {
            hipLaunchKernelGGL(record_flag_facts_kernel, dim3(grid_for(records, kThreads)), dim3(kThreads), 0, stream, (const int *)pos_dev,
                               (const unsigned short *)flag_dev, offsets_dev, (int)T, mapped_dev, unsorted_dev);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(mapped.data(), mapped_dev, T * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(unsorted.data(), unsorted_dev, T * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t t = 0; t < T; ++t) {
        mapped_out_host[t] = (int64_t)mapped[t];
        unsorted_out_host[t] = unsorted[t];
    }
    return ROCCO_HIP_OK;
}

size_t fragment_block_centers_scratch_bytes(const int64_t *rec_offsets_host, size_t T, const int64_t *contig_len_host, int block_size,
                                            int rolling_chunk_size)
{
    if (check_record_tracks(rec_offsets_host, T, "fragment_block_centers") != ROCCO_HIP_OK || block_size < 64 || rolling_chunk_size < 1) {
        return 0;
    }
    const long long max_chunks = max_chunks_of(contig_len_host, T, block_size, rolling_chunk_size);
    if (max_chunks >= 0x7ffffffeLL) {
        set_last_error("fragment_block_centers: a contig has 2^31 chunks or more");
        return 0;
    }
    size_t cub_bytes = 0;
    if (size_centers_cub(max_chunks, cub_bytes) != ROCCO_HIP_OK) {
        return 0;
    }
    return CentersLayout((size_t)max_chunks, cub_bytes).bytes;
}

int launch_fragment_block_centers(const int32_t *pos_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t T,
                                  const int64_t *contig_len_host, int flag_exclude, int max_iterations, int block_size,
                                  int rolling_chunk_size, int32_t *centers_out_host, int32_t *center_count_out_host,
                                  const int64_t *chunk_offsets_host, int32_t *density_out_dev, int32_t *rank_out_dev, void *scratch_dev,
                                  hipStream_t stream)
{
    if (max_iterations < 1 || block_size < 64 || rolling_chunk_size < 1 ||
        ((density_out_dev != nullptr || rank_out_dev != nullptr) && chunk_offsets_host == nullptr)) {
        set_last_error("fragment_block_centers: parameters below the reference's clamps, or outputs without their offsets");
        return ROCCO_HIP_EINVAL;
    }
    int rc = check_record_tracks(rec_offsets_host, T, "fragment_block_centers");
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    const long long max_chunks = max_chunks_of(contig_len_host, T, block_size, rolling_chunk_size);
    size_t cub_size = 0;
    if (max_chunks >= 0x7ffffffeLL || (rc = size_centers_cub(max_chunks, cub_size)) != ROCCO_HIP_OK) {
        return max_chunks >= 0x7ffffffeLL ? ROCCO_HIP_EINVAL : rc;
    }
    const CentersLayout lay((size_t)max_chunks, cub_size);
    char *sc = (char *)scratch_dev;
    int *raw = (int *)(sc + lay.raw), *prefix = (int *)(sc + lay.prefix), *density = (int *)(sc + lay.density);
    int *index = (int *)(sc + lay.index), *density_sorted = (int *)(sc + lay.density_sorted);
    int *index_sorted = (int *)(sc + lay.index_sorted);
    int win_size = block_size / rolling_chunk_size;  // ccounts_backend.c:1274-1283
    if (win_size < 1) {
        win_size = 1;
    }
    if ((win_size & 1) == 0) {
        win_size += 1;
    }
    const int win_half = win_size / 2;
    std::vector<int> values, indices;
    std::vector<bool> seen;
    for (size_t t = 0; t < T; ++t) {
        center_count_out_host[t] = 0;
        const long long chunks = chunks_of(contig_len_host[t], block_size, rolling_chunk_size);
        if (chunks == 0) {
            if (chunk_offsets_host != nullptr && chunk_offsets_host[t + 1] != chunk_offsets_host[t]) {
                set_last_error("fragment_block_centers: chunk offsets do not match the contigs");
                return ROCCO_HIP_EINVAL;
            }
            continue;
        }
        if (chunk_offsets_host != nullptr && chunk_offsets_host[t + 1] - chunk_offsets_host[t] != chunks) {
            set_last_error("fragment_block_centers: chunk offsets do not match the contigs");
            return ROCCO_HIP_EINVAL;
        }
        const int n = (int)chunks;
        const long long lo = rec_offsets_host[t], hi = rec_offsets_host[t + 1];
        ROCCO_HIP_TRY(hipMemsetAsync(raw, 0, ((size_t)n + 1) * sizeof(int), stream));
        if (hi > lo) {
            hipLaunchKernelGGL(chunk_density_kernel, dim3(grid_for(hi - lo, kDensityRecords)), dim3(kThreads), 0, stream,
                               (const int *)pos_dev, (const unsigned short *)flag_dev, lo, hi, flag_exclude, rolling_chunk_size,
                               (long long)contig_len_host[t], n, raw);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        size_t cub_bytes = cub_size;
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + lay.cub, cub_bytes, (const int *)raw, prefix, n + 1, stream));
        hipLaunchKernelGGL(window_sums_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           (const int *)prefix, n, win_size, density, index);
        ROCCO_HIP_TRY(hipGetLastError());
        cub_bytes = cub_size;
        ROCCO_HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(sc + lay.cub, cub_bytes, (const int *)density, density_sorted,
                                                                   (const int *)index, index_sorted, n, 0, 32, stream));
        if (density_out_dev != nullptr) {
            ROCCO_HIP_TRY(hipMemcpyAsync(density_out_dev + chunk_offsets_host[t], density, (size_t)n * sizeof(int),
                                         hipMemcpyDeviceToDevice, stream));
        }
        if (rank_out_dev != nullptr) {
            ROCCO_HIP_TRY(hipMemcpyAsync(rank_out_dev + chunk_offsets_host[t], index_sorted, (size_t)n * sizeof(int),
                                         hipMemcpyDeviceToDevice, stream));
        }
        // ccounts_backend.c:1314-1339 over a prefix of the ranking, extended while it runs out
        const int take = max_iterations < n ? max_iterations : n;
        seen.assign((size_t)n, false);
        int32_t *centers = centers_out_host + t * (size_t)max_iterations;
        int accepted = 0, have = 0, at = 0;
        bool done = false;
        while (!done) {
            if (at == have) {
                if (have == n) {
                    break;
                }
                long long more = (long long)take * (win_size < 4096 ? win_size : 4096) + 1024;
                more = more < have ? have : more;  // (at least doubling)
                const int upto = (int)((long long)have + more < n ? (long long)have + more : n);
                values.resize((size_t)upto);
                indices.resize((size_t)upto);
                const int copied = queue_then_drain(stream, [&]() -> int {  // (into `values` and `indices`)
                    ROCCO_HIP_TRY(hipMemcpyAsync(values.data() + have, density_sorted + have, (size_t)(upto - have) * sizeof(int),
                                                 hipMemcpyDeviceToHost, stream));
                    ROCCO_HIP_TRY(hipMemcpyAsync(indices.data() + have, index_sorted + have, (size_t)(upto - have) * sizeof(int),
                                                 hipMemcpyDeviceToHost, stream));
                    ROCCO_HIP_TRY(hipStreamSynchronize(stream));
                    return ROCCO_HIP_OK;
                });
                if (copied != ROCCO_HIP_OK) {
                    return copied;
                }
                have = upto;
            }
            for (; at < have; ++at) {
                if (accepted >= take || values[at] <= 0) {  // (descending: nothing positive follows)
                    done = true;
                    break;
                }
                const int center = indices[at];
                if (center < 0 || center >= n || seen[(size_t)center]) {
                    continue;
                }
                centers[accepted++] = center;
                int s = center - win_half, e = s + win_size;
                s = s < 0 ? 0 : s;
                e = e > n ? n : e;
                for (int i = s; i < e; ++i) {
                    seen[(size_t)i] = true;
                }
            }
        }
        center_count_out_host[t] = accepted;
    }
    ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // the scratch buffer is the solver's
    return ROCCO_HIP_OK;
}

size_t strand_xcorr_scratch_bytes(size_t T, size_t n_blocks) { return XcorrLayout(T, n_blocks).bytes; }

int launch_strand_xcorr_blocks(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host,
                               size_t T, const int32_t *block_track_host, const int64_t *block_start_host, size_t n_blocks,
                               const int32_t *min_lag_host, int flag_exclude, int block_size, int max_insert_size, int lag_step,
                               int32_t *best_lag_out_host, double *best_score_out_host, int32_t *fwd_sum_out_host,
                               int32_t *rev_sum_out_host, void *scratch_dev, hipStream_t stream)
{
    int rc = check_record_tracks(rec_offsets_host, T, "strand_xcorr_blocks");
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    if (block_size < 64 || block_size > kMaxBlockSize || max_insert_size < 1 || lag_step < 1 || n_blocks == 0 ||
        n_blocks >= (size_t)0x7fffffff) {
        set_last_error("strand_xcorr_blocks: block_size outside [64, " + std::to_string(kMaxBlockSize) +
                       "] (two int32 arrays of a block must fit a workgroup's LDS), or another parameter below the reference's clamps");
        return ROCCO_HIP_EINVAL;
    }
    for (size_t t = 0; t < T; ++t) {
        if (min_lag_host[t] < 1) {
            set_last_error("strand_xcorr_blocks: a track's smallest lag is below 1");
            return ROCCO_HIP_EINVAL;
        }
    }
    for (size_t b = 0; b < n_blocks; ++b) {
        if (block_track_host[b] < 0 || (size_t)block_track_host[b] >= T || block_start_host[b] < 0 ||
            block_start_host[b] + block_size > (1LL << 31)) {
            set_last_error("strand_xcorr_blocks: a block names no track or leaves [0, 2^31)");
            return ROCCO_HIP_EINVAL;
        }
    }
    std::vector<long long> offsets(rec_offsets_host, rec_offsets_host + T + 1), starts(block_start_host, block_start_host + n_blocks);
    std::vector<int> best_lag(n_blocks), fwd_sum(n_blocks), rev_sum(n_blocks);
    std::vector<double> best_score(n_blocks);
    const XcorrLayout at(T, n_blocks);
    char *sc = (char *)scratch_dev;
    long long *offsets_dev = (long long *)(sc + at.rec_offsets), *start_dev = (long long *)(sc + at.block_start);
    int *min_lag_dev = (int *)(sc + at.min_lag), *track_dev = (int *)(sc + at.block_track);
    int *lag_dev = (int *)(sc + at.best_lag), *fwd_dev = (int *)(sc + at.fwd_sum), *rev_dev = (int *)(sc + at.rev_sum);
    double *score_dev = (double *)(sc + at.best_score);
    const size_t lds_bytes = (size_t)block_size * 2 * sizeof(int);
    const int queued = queue_then_drain(stream, [&]() -> int {  // (the caller's arrays and this call's vectors are read and written)
        ROCCO_HIP_TRY(hipFuncSetAttribute((const void *)strand_xcorr_blocks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds_bytes));
        ROCCO_HIP_TRY(hipMemcpyAsync(offsets_dev, offsets.data(), (T + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(min_lag_dev, min_lag_host, T * sizeof(int), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(track_dev, block_track_host, n_blocks * sizeof(int), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(start_dev, starts.data(), n_blocks * sizeof(long long), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(strand_xcorr_blocks_kernel, dim3((unsigned)n_blocks), dim3(kThreads), lds_bytes, stream, (const int *)pos_dev,
                           (const int *)end_dev, (const unsigned short *)flag_dev, offsets_dev, track_dev, start_dev, min_lag_dev,
                           flag_exclude, block_size, max_insert_size, lag_step, lag_dev, score_dev, fwd_dev, rev_dev);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(best_lag.data(), lag_dev, n_blocks * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(fwd_sum.data(), fwd_dev, n_blocks * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(rev_sum.data(), rev_dev, n_blocks * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(best_score.data(), score_dev, n_blocks * sizeof(double), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t b = 0; b < n_blocks; ++b) {
        best_lag_out_host[b] = best_lag[b];
        best_score_out_host[b] = best_score[b];
        fwd_sum_out_host[b] = fwd_sum[b];
        rev_sum_out_host[b] = rev_sum[b];
    }
    return ROCCO_HIP_OK;
}

namespace {

int size_select(long long most, size_t &bytes)
{
    bytes = 0;
    if (hipcub::DeviceSelect::If(nullptr, bytes, (const int *)nullptr, (int *)nullptr, (int *)nullptr, (int)most, NotNegative()) !=
        hipSuccess) {
        (void)hipGetLastError();
        set_last_error("template_lengths: cannot size the compaction");
        return ROCCO_HIP_EHIP;
    }
    return ROCCO_HIP_OK;
}

long long most_records(const int64_t *rec_offsets_host, size_t T)
{
    long long most = 1;
    for (size_t t = 0; t < T; ++t) {
        const long long n = rec_offsets_host[t + 1] - rec_offsets_host[t];
        most = n > most ? n : most;
    }
    return most;
}

}  // namespace

size_t template_lengths_scratch_bytes(const int64_t *rec_offsets_host, size_t T)
{
    size_t select_bytes = 0;
    if (check_record_tracks(rec_offsets_host, T, "template_lengths") != ROCCO_HIP_OK ||
        size_select(most_records(rec_offsets_host, T), select_bytes) != ROCCO_HIP_OK) {
        return 0;
    }
    return TemplateLayout(T, select_bytes).bytes;
}

int launch_template_lengths(const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mate_same_dev,
                            const int64_t *rec_offsets_host, size_t T, const int32_t *min_insert_host, int flag_exclude,
                            int max_insert_size, int32_t *lengths_tmp_dev, int32_t *lengths_out_dev, int64_t *count_out_host,
                            void *scratch_dev, hipStream_t stream)
{
    int rc = check_record_tracks(rec_offsets_host, T, "template_lengths");
    size_t select_bytes = 0;
    if (rc != ROCCO_HIP_OK || (rc = size_select(most_records(rec_offsets_host, T), select_bytes)) != ROCCO_HIP_OK) {
        return rc;
    }
    std::vector<long long> offsets(rec_offsets_host, rec_offsets_host + T + 1);
    std::vector<int> counts(T, 0);
    const long long records = offsets[T] - offsets[0];
    const TemplateLayout at(T, select_bytes);
    char *sc = (char *)scratch_dev;
    long long *offsets_dev = (long long *)(sc + at.rec_offsets);
    int *min_insert_dev = (int *)(sc + at.min_insert), *counts_dev = (int *)(sc + at.counts);
    char *select_dev = sc + at.select;
    const int queued = queue_then_drain(stream, [&]() -> int {  // (this call's vectors go up and `counts` comes back)
        ROCCO_HIP_TRY(hipMemcpyAsync(offsets_dev, offsets.data(), (T + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(min_insert_dev, min_insert_host, T * sizeof(int), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(counts_dev, 0, T * sizeof(int), stream));
        if (records > 0) {
            hipLaunchKernelGGL(template_length_kernel, dim3(grid_for(records, kThreads)), dim3(kThreads), 0, stream,
                               (const int *)isize_dev, (const unsigned short *)flag_dev, (const unsigned char *)mate_same_dev,
                               offsets_dev, (int)T, min_insert_dev, flag_exclude, max_insert_size, (int *)lengths_tmp_dev);
            ROCCO_HIP_TRY(hipGetLastError());
            for (size_t t = 0; t < T; ++t) {
                const long long n = offsets[t + 1] - offsets[t];
                if (n > 0) {
                    size_t bytes = select_bytes;
                    ROCCO_HIP_TRY(hipcub::DeviceSelect::If(select_dev, bytes, (const int *)lengths_tmp_dev + offsets[t],
                                                           (int *)lengths_out_dev + offsets[t], counts_dev + t, (int)n, NotNegative(),
                                                           stream));
                }
            }
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(counts.data(), counts_dev, T * sizeof(int), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t t = 0; t < T; ++t) {
        count_out_host[t] = counts[t];
    }
    return ROCCO_HIP_OK;
}

}  // namespace rocco
