// rocco_amd/csrc/fragments_file.hip -- the inflated text of fragments files -> lines -> fields -> bins in HBM, gfx950
// (note (34)).  The rules are fragments_rules.h's, the same source the host twin compiles.
//
// lines: a facts kernel counts the '\n' of every tile of ROCCO_FRAGFILE_TILE_BYTES bytes (16 bytes per lane; one 16-byte
//   load where the address allows it) and keeps the offset behind the last one; hipcub's exclusive sum over the tiles gives
//   every tile its first line; an emit kernel repeats the count per lane, scans the lanes of the tile and writes the starts.
// fields: one lane per line walks its bytes once (fragline_parse); a second kernel compares every line's start with that of
//   the line before it in its track.  The first offending line and its lowest code come back through one 64-bit atomicMin.
// count: one lane per line adds its weight to at most two cells of its track's positive sums P and, for coverage, to one
//   cell of its negative sums N (64-bit integer atomics in HBM; no LDS window: a pile of fragments in one bin meets at
//   one L2 atomic unit, which is what DESIGN.md note (34) leaves unmeasured); a finish kernel, one workgroup per track,
//   scans P - N tile by tile with hipcub's block scan, or copies P, converts once to float32 and keeps the largest magnitude.
// range, mapped count: one lane per line, atomicMin / atomicMax of the qualifying line indices per track, an integer sum.
// Bound: every pass reads its inputs once; the text is read twice by the line pass and once by the field pass.
#include <hipcub/hipcub.hpp>

#include "fragments_rules.h"
#include "kernels.h"

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_FRAGFILE_THREADS;
constexpr int kLaneBytes = ROCCO_FRAGFILE_TILE_BYTES / ROCCO_FRAGFILE_THREADS;
constexpr int kScanItems = ROCCO_FRAGFILE_SCAN_ITEMS;
static_assert(kLaneBytes == 16, "a lane takes one 16-byte load of its tile");

// the '\n' among the 16 bytes of a lane that begin a line behind them: those at p with entry0 <= p and p + 1 < n_bytes.
// `mask` has bit j set for such a byte at p0 + j; returns (through last) the offset behind the last '\n' at p < n_bytes.
__device__ unsigned lane_newlines(const uint8_t *__restrict__ bytes, long long n_bytes, long long entry0, long long p0, long long *last)
{
    uint8_t b[kLaneBytes];
    if (p0 >= entry0 && p0 + kLaneBytes <= n_bytes && (((uintptr_t)(bytes + p0)) & 15u) == 0) {
        const uint4 v = *(const uint4 *)(bytes + p0);
        memcpy(b, &v, sizeof(v));
    } else {
        for (int j = 0; j < kLaneBytes; ++j) {
            const long long p = p0 + j;
            b[j] = (p >= entry0 && p < n_bytes) ? bytes[p] : (uint8_t)0;
        }
    }
    unsigned mask = 0;
    for (int j = 0; j < kLaneBytes; ++j) {
        const long long p = p0 + j;
        if (b[j] == '\n' && p >= entry0 && p < n_bytes) {
            *last = p + 1;
            if (p + 1 < n_bytes) {
                mask |= 1u << j;
            }
        }
    }
    return mask;
}

__global__ __launch_bounds__(kThreads) void fragfile_line_facts_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, long long entry0,
                                                                       long long tile0, long long n_tiles, long long *__restrict__ counts,
                                                                       unsigned long long *__restrict__ cut)
{
    using Reduce = hipcub::BlockReduce<long long, kThreads>;
    __shared__ typename Reduce::TempStorage temp;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        long long last = 0;
        const unsigned mask = lane_newlines(bytes, n_bytes, entry0, (tile0 + t) * ROCCO_FRAGFILE_TILE_BYTES + (long long)threadIdx.x * kLaneBytes, &last);
        const long long total = Reduce(temp).Sum((long long)__popc(mask));
        __syncthreads();
        const long long behind = Reduce(temp).Reduce(last, hipcub::Max());
        __syncthreads();
        if (threadIdx.x == 0) {
            counts[t] = total;
            if (behind > 0) {
                atomicMax(cut, (unsigned long long)behind);
            }
        }
    }
}

// tile_first: the exclusive sum of the n_tiles + 1 counts (the last is 0), so tile_first[n_tiles] is the number of starts
// behind the first
__global__ __launch_bounds__(kThreads) void fragfile_line_emit_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, long long entry0,
                                                                      long long tile0, long long n_tiles, const long long *__restrict__ tile_first,
                                                                      long long *__restrict__ starts, long long capacity)
{
    using Scan = hipcub::BlockScan<int, kThreads>;
    __shared__ typename Scan::TempStorage temp;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long first = entry0 < n_bytes ? 1 : 0, n_lines = first + (n_tiles > 0 ? tile_first[n_tiles] : 0);
        if (first && capacity > 0) {
            starts[0] = entry0;
        }
        if (n_lines < capacity) {
            starts[n_lines] = n_bytes;
        }
    }
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        long long last = 0;
        const long long p0 = (tile0 + t) * ROCCO_FRAGFILE_TILE_BYTES + (long long)threadIdx.x * kLaneBytes;
        unsigned mask = lane_newlines(bytes, n_bytes, entry0, p0, &last);
        int before = 0;
        Scan(temp).ExclusiveSum(__popc(mask), before);
        __syncthreads();
        long long to = 1 + tile_first[t] + before;
        while (mask != 0) {
            const int j = __ffs(mask) - 1;
            mask &= mask - 1;
            if (to >= 0 && to < capacity) {
                starts[to] = p0 + j + 1;
            }
            ++to;
        }
    }
}

struct FieldTracks {
    const int64_t *first;       // K + 1 line offsets
    const int32_t *expect;      // K
    const int64_t *allow_first; // K + 1
    long long K;
};

__global__ __launch_bounds__(kThreads) void fragfile_fields_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, const int64_t *__restrict__ starts,
                                                                   long long n_lines, int whole_file, FieldTracks tracks, FragNames names,
                                                                   const uint8_t *__restrict__ allow_bytes, const int64_t *__restrict__ allow_offsets,
                                                                   int32_t *__restrict__ start_out, int32_t *__restrict__ end_out,
                                                                   int32_t *__restrict__ weight_out, int32_t *__restrict__ name_out,
                                                                   uint32_t *__restrict__ status_out, unsigned long long *__restrict__ first_error)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (long long)gridDim.x * kThreads) {
        const long long at = starts[i], next = starts[i + 1];
        const long long k = frag_track(tracks.first, tracks.K, i);
        FragLine line = {0, 0, 1, -1, 0u, ROCCO_FRAGFILE_ERR_FIELDS};
        if (at >= 0 && at <= next && next <= n_bytes) {  // (starts that are not this buffer's: nothing of it is read)
            const FragNames allow = {allow_bytes, allow_offsets, tracks.allow_first[k], tracks.allow_first[k + 1]};
            line = fragline_parse(bytes + at, next - at, whole_file, names, allow);
        }
        start_out[i] = line.start;
        end_out[i] = line.end;
        weight_out[i] = line.weight;
        name_out[i] = line.name;
        status_out[i] = line.status;
        const int error = frag_line_error(line, whole_file, tracks.expect[k]);
        if (error != 0) {
            atomicMin(first_error, ((unsigned long long)i << 32) | (unsigned long long)(unsigned)error);
        }
    }
}

// a span's line whose start lies below that of the line before it in its track (meta lines and refused lines passed over)
__global__ __launch_bounds__(kThreads) void fragfile_order_kernel(const int32_t *__restrict__ start, const uint32_t *__restrict__ status,
                                                                  long long n_lines, FieldTracks tracks, unsigned long long *__restrict__ first_error)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (long long)gridDim.x * kThreads) {
        if (!frag_span_ok(status[i])) {
            continue;
        }
        const long long first = tracks.first[frag_track(tracks.first, tracks.K, i)];
        long long j = i - 1;
        while (j >= first && !frag_span_ok(status[j])) {
            --j;
        }
        if (j >= first && start[j] > start[i]) {
            atomicMin(first_error, ((unsigned long long)i << 32) | (unsigned long long)ROCCO_FRAGFILE_ERR_ORDER);
        }
    }
}

__global__ void fragfile_report_kernel(const unsigned long long *__restrict__ first_error, long long *__restrict__ back)
{
    const unsigned long long packed = *first_error;
    const bool none = packed == ~0ULL;
    back[0] = none ? -1 : (long long)(packed >> 32);
    back[1] = none ? 0 : (long long)(packed & 0xffffffffULL);
    back[2] = back[3] = 0;
}

// a track of the count, range and finish kernels
struct FragTrack {
    long long cells_first, out_offset;
    int start, end, step, n_bins, mode, one_read_per_bin;
};

__global__ __launch_bounds__(kThreads) void fragfile_count_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end,
                                                                  const int32_t *__restrict__ weight, const uint32_t *__restrict__ status,
                                                                  const int64_t *__restrict__ line_first, const FragTrack *__restrict__ tracks,
                                                                  long long K, unsigned long long *__restrict__ P, unsigned long long *__restrict__ N)
{
    const long long base = line_first[0], n = line_first[K] - base;
    for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < n; u += (long long)gridDim.x * kThreads) {
        const long long i = base + u;
        const uint32_t s = status[i];
        const int32_t a = start[i], b = end[i];
        if (!frag_valid_count(s, a, b)) {
            continue;
        }
        const FragTrack t = tracks[frag_track(line_first, K, i)];
        const FragCells c = frag_cells(a, b, t.mode, t.one_read_per_bin, t.start, t.end, t.step, t.n_bins);
        const unsigned long long w = (unsigned long long)weight[i];
        for (int q = 0; q < c.n_plus; ++q) {
            atomicAdd(P + t.cells_first + c.plus[q], w);
        }
        if (c.minus >= 0) {
            atomicAdd(N + t.cells_first + c.minus, w);
        }
    }
}

// one workgroup per track: out = float32(the running sum of P - N) for coverage without one_read_per_bin, float32(P) otherwise
__global__ __launch_bounds__(kThreads) void fragfile_finish_kernel(const FragTrack *__restrict__ tracks, long long K,
                                                                   const unsigned long long *__restrict__ P, const unsigned long long *__restrict__ N,
                                                                   float *__restrict__ out, long long *__restrict__ maxima)
{
    using Scan = hipcub::BlockScan<long long, kThreads>;
    using Reduce = hipcub::BlockReduce<long long, kThreads>;
    __shared__ typename Scan::TempStorage scan_temp;
    __shared__ typename Reduce::TempStorage reduce_temp;
    __shared__ long long carry_shared;
    for (long long k = blockIdx.x; k < K; k += gridDim.x) {
        const FragTrack t = tracks[k];
        const bool running = t.mode == ROCCO_FRAGFILE_MODE_COVERAGE && !t.one_read_per_bin;
        long long carry = 0, largest = 0;
        for (long long tile = 0; tile < t.n_bins; tile += (long long)kThreads * kScanItems) {
            const long long b0 = tile + (long long)threadIdx.x * kScanItems;
            long long v[kScanItems], sum = 0;
            for (int q = 0; q < kScanItems; ++q) {
                const long long b = b0 + q;
                long long p = 0, m = 0;
                if (b < t.n_bins) {
                    p = (long long)P[t.cells_first + b];
                    m = (long long)N[t.cells_first + b];
                }
                largest = max(largest, max(p, m));
                v[q] = running ? p - m : p;
                sum += v[q];
            }
            long long before = 0, total = 0;
            if (running) {
                Scan(scan_temp).ExclusiveSum(sum, before, total);
            }
            long long value = carry + before;
            for (int q = 0; q < kScanItems; ++q) {
                const long long b = b0 + q;
                value = running ? value + v[q] : v[q];
                if (b < t.n_bins) {
                    largest = max(largest, value < 0 ? -value : value);
                    out[t.out_offset + b] = (float)value;
                }
            }
            if (running) {
                if (threadIdx.x == 0) {
                    carry_shared = carry + total;
                }
                __syncthreads();
                carry = carry_shared;
                __syncthreads();
            }
        }
        if (running && threadIdx.x == 0 && t.n_bins >= 0) {
            largest = max(largest, (long long)N[t.cells_first + t.n_bins]);  // (the cell behind the last bin)
        }
        const long long most = Reduce(reduce_temp).Reduce(largest, hipcub::Max());
        __syncthreads();
        if (threadIdx.x == 0) {
            maxima[k] = most;
        }
    }
}

__global__ __launch_bounds__(kThreads) void fragfile_range_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end,
                                                                  const uint32_t *__restrict__ status, const int64_t *__restrict__ line_first,
                                                                  const int64_t *__restrict__ chrom_len, long long K,
                                                                  unsigned long long *__restrict__ first, unsigned long long *__restrict__ last)
{
    const long long base = line_first[0], n = line_first[K] - base;
    for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < n; u += (long long)gridDim.x * kThreads) {
        const long long i = base + u;
        if (frag_valid_range(status[i], start[i], end[i])) {
            const long long k = frag_track(line_first, K, i);
            if (start[i] >= chrom_len[k]) {  // (the query over [0, chrom_len) does not yield the line)
                continue;
            }
            atomicMin(first + k, (unsigned long long)i);
            atomicMax(last + k, (unsigned long long)i + 1);
        }
    }
}

__global__ void fragfile_range_fetch_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ end, long long K,
                                            const unsigned long long *__restrict__ first, const unsigned long long *__restrict__ last,
                                            long long *__restrict__ range)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) {
        range[2 * k] = first[k] == ~0ULL ? 0 : (long long)start[first[k]];
        range[2 * k + 1] = last[k] == 0 ? 0 : (long long)end[last[k] - 1];
    }
}

__global__ __launch_bounds__(kThreads) void fragfile_mapped_kernel(const int32_t *__restrict__ weight, const int32_t *__restrict__ name,
                                                                   const uint32_t *__restrict__ status, long long n_lines, int mode,
                                                                   int one_read_per_bin, unsigned long long *__restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<unsigned long long, kThreads>;
    __shared__ typename Reduce::TempStorage temp;
    unsigned long long mine = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (long long)gridDim.x * kThreads) {
        if (frag_valid_mapped(status[i], name[i])) {
            mine += (unsigned long long)frag_mapped_weight(weight[i], mode, one_read_per_bin);
        }
    }
    const unsigned long long total = Reduce(temp).Sum(mine);
    if (threadIdx.x == 0 && total != 0) {
        atomicAdd(sum, total);
    }
}

unsigned capped_grid(long long units, int cap) { return (unsigned)(units < 1 ? 1 : (units < (long long)cap ? units : (long long)cap)); }

long long line_tiles(size_t n_bytes, size_t entry0, long long *tile0)
{
    *tile0 = (long long)(entry0 / ROCCO_FRAGFILE_TILE_BYTES);
    return n_bytes > entry0 ? (long long)((n_bytes + ROCCO_FRAGFILE_TILE_BYTES - 1) / ROCCO_FRAGFILE_TILE_BYTES) - *tile0 : 0;
}

size_t tiles_scan_bytes(long long n_tiles)
{
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const long long *)nullptr, (long long *)nullptr, (int)(n_tiles + 1)) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes > 0 ? bytes : 1;
}

// fragfile_lines: the n_tiles + 1 counts, their exclusive sum, the offset behind the last '\n', what comes back, hipcub's scan
struct LinesLayout {
    size_t counts, tile_first, cut, scan, bytes;
    LinesLayout(long long n_tiles, size_t scan_bytes)
    {
        Layout lay;
        counts = lay.at((size_t)(n_tiles + 1) * sizeof(long long));
        tile_first = lay.at((size_t)(n_tiles + 1) * sizeof(long long));
        cut = lay.at(sizeof(unsigned long long));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

// fragfile_fields: what goes up in one copy (K + 1 line offsets, K + 1 allow-list offsets, n_names + 1 name offsets as int64;
// K expected names as int32; the names' bytes), the word of the first offending line, the report
struct FieldsLayout {
    size_t track_first, allow_first, name_offsets, expect, names, uploaded, first_error, back, bytes;
    FieldsLayout(size_t K, size_t n_names, size_t name_bytes)
    {
        Layout lay;
        track_first = lay.at((K + 1) * sizeof(int64_t));
        allow_first = lay.at((K + 1) * sizeof(int64_t));
        name_offsets = lay.at((n_names + 1) * sizeof(int64_t));
        expect = lay.at(K * sizeof(int32_t));
        names = lay.at(name_bytes > 0 ? name_bytes : 1);
        uploaded = lay.bytes();
        first_error = lay.at(sizeof(unsigned long long));
        back = lay.at(4 * sizeof(long long));
        bytes = lay.bytes();
    }
};

// fragfile_count_batch / _chrom_range_batch: the K + 1 line offsets and the K tracks (the range: K chromosome lengths; one copy), per track its largest
// magnitude or its first / last line and the 2 K values that go back, then P and N (zeroed with one memset: the tail)
struct TracksLayout {
    size_t line_first, tracks, uploaded, maxima, first, last, cells, bytes;
    TracksLayout(size_t K, size_t n_cells)
    {
        Layout lay;
        line_first = lay.at((K + 1) * sizeof(int64_t));
        tracks = lay.at((K * sizeof(FragTrack) > K * sizeof(int64_t) ? K * sizeof(FragTrack) : K * sizeof(int64_t)));
        uploaded = lay.bytes();
        maxima = lay.at(2 * K * sizeof(long long));
        first = lay.at(K * sizeof(unsigned long long));
        last = lay.at(K * sizeof(unsigned long long));
        cells = lay.at(2 * n_cells * sizeof(unsigned long long));
        bytes = lay.bytes();
    }
};

bool offsets_ascend(const int64_t *offsets, size_t K)
{
    if (offsets[0] < 0) {
        return false;
    }
    for (size_t k = 0; k < K; ++k) {
        if (offsets[k] > offsets[k + 1]) {
            return false;
        }
    }
    return true;
}

}  // namespace

size_t fragfile_lines_scratch_bytes(size_t n_bytes, size_t entry0)
{
    long long tile0;
    const long long n_tiles = line_tiles(n_bytes, entry0, &tile0);
    const size_t scan = tiles_scan_bytes(n_tiles);
    return scan == 0 ? 0 : LinesLayout(n_tiles, scan).bytes;
}

int launch_fragfile_lines(const uint8_t *bytes_dev, size_t n_bytes, size_t entry0, int64_t *starts_out_dev, size_t capacity,
                          int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    long long tile0;
    const long long n_tiles = line_tiles(n_bytes, entry0, &tile0);
    const LinesLayout at(n_tiles, tiles_scan_bytes(n_tiles));
    char *sc = (char *)scratch_dev;
    long long *counts = (long long *)(sc + at.counts), *tile_first = (long long *)(sc + at.tile_first);
    unsigned long long *cut = (unsigned long long *)(sc + at.cut);
    size_t scan_bytes = at.bytes - at.scan;
    long long total = 0;
    unsigned long long behind = 0;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(cut, 0, sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(counts + n_tiles, 0, sizeof(long long), stream));
        if (n_tiles > 0) {
            hipLaunchKernelGGL(fragfile_line_facts_kernel, dim3(capped_grid(n_tiles, ROCCO_FRAGFILE_LINES_MAX_GRID)), dim3(kThreads), 0, stream,
                               bytes_dev, (long long)n_bytes, (long long)entry0, tile0, n_tiles, counts, cut);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const long long *)counts, tile_first, (int)(n_tiles + 1), stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(&total, tile_first + n_tiles, sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(&behind, cut, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the size the caller allocates from, and the error state of the kernels above)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    const long long n_lines = total + (entry0 < n_bytes ? 1 : 0);
    report_out_host[0] = n_lines;
    report_out_host[1] = behind > 0 ? (long long)behind : (long long)entry0;
    report_out_host[2] = (entry0 < n_bytes && (long long)behind != (long long)n_bytes) ? 1 : 0;
    report_out_host[3] = 0;
    if (starts_out_dev == nullptr) {
        return ROCCO_HIP_OK;
    }
    if (capacity < (size_t)n_lines + 1) {
        set_last_error("fragfile_lines: the bytes hold " + std::to_string(n_lines) + " lines, starts_out_dev has room for " +
                       std::to_string(capacity) + " entries where one more than the lines belong");
        return ROCCO_HIP_EINVAL;
    }
    return queue_then_drain(stream, [&]() -> int {
        hipLaunchKernelGGL(fragfile_line_emit_kernel, dim3(capped_grid(n_tiles, ROCCO_FRAGFILE_LINES_MAX_GRID)), dim3(kThreads), 0, stream, bytes_dev,
                           (long long)n_bytes, (long long)entry0, tile0, n_tiles, (const long long *)tile_first, (long long *)starts_out_dev,
                           (long long)capacity);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (a fault of this kernel is this call's error)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
}

size_t fragfile_fields_scratch_bytes(size_t K, size_t n_names, size_t name_bytes) { return FieldsLayout(K, n_names, name_bytes).bytes; }

int launch_fragfile_fields(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines, int whole_file,
                           const int64_t *track_first_host, const int32_t *expect_host, size_t K, const uint8_t *names_host,
                           const int64_t *name_offsets_host, size_t n_names, const uint8_t *allow_bytes_dev, const int64_t *allow_offsets_dev,
                           size_t n_allow, const int64_t *allow_first_host, int32_t *start_out_dev, int32_t *end_out_dev, int32_t *weight_out_dev,
                           int32_t *name_out_dev, uint32_t *status_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    if (!offsets_ascend(track_first_host, K) || track_first_host[0] != 0 || track_first_host[K] != (int64_t)n_lines ||
        !offsets_ascend(allow_first_host, K) || allow_first_host[K] > (int64_t)n_allow || !offsets_ascend(name_offsets_host, n_names)) {
        set_last_error("fragfile_fields: track_first_host must ascend from 0 to n_lines, allow_first_host within the n_allow entries, "
                       "name_offsets_host from a non-negative begin");
        return ROCCO_HIP_EINVAL;
    }
    for (size_t k = 0; k < K; ++k) {
        if (expect_host[k] >= (int32_t)n_names) {
            set_last_error("fragfile_fields: expect_host names an entry the name table does not have");
            return ROCCO_HIP_EINVAL;
        }
    }
    const size_t name_bytes = (size_t)name_offsets_host[n_names];
    const FieldsLayout at(K, n_names, name_bytes);
    std::vector<char> staged(at.uploaded, 0);
    memcpy(staged.data() + at.track_first, track_first_host, (K + 1) * sizeof(int64_t));
    memcpy(staged.data() + at.allow_first, allow_first_host, (K + 1) * sizeof(int64_t));
    memcpy(staged.data() + at.name_offsets, name_offsets_host, (n_names + 1) * sizeof(int64_t));
    memcpy(staged.data() + at.expect, expect_host, K * sizeof(int32_t));
    if (name_bytes > 0) {
        memcpy(staged.data() + at.names, names_host, name_bytes);
    }
    char *sc = (char *)scratch_dev;
    unsigned long long *first_error = (unsigned long long *)(sc + at.first_error);
    long long back[4] = {-1, 0, 0, 0};
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemcpyAsync(sc, staged.data(), staged.size(), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(first_error, 0xff, sizeof(unsigned long long), stream));
        const FieldTracks tracks = {(const int64_t *)(sc + at.track_first), (const int32_t *)(sc + at.expect),
                                    (const int64_t *)(sc + at.allow_first), (long long)K};
        const FragNames names = {(const uint8_t *)(sc + at.names), (const int64_t *)(sc + at.name_offsets), 0, (long long)n_names};
        if (n_lines > 0) {
            const unsigned grid = capped_grid((long long)((n_lines + kThreads - 1) / kThreads), ROCCO_FRAGFILE_FIELDS_MAX_GRID);
            hipLaunchKernelGGL(fragfile_fields_kernel, dim3(grid), dim3(kThreads), 0, stream, bytes_dev, (long long)n_bytes, starts_dev,
                               (long long)n_lines, whole_file, tracks, names, allow_bytes_dev, allow_offsets_dev, start_out_dev, end_out_dev,
                               weight_out_dev, name_out_dev, status_out_dev, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            if (!whole_file) {
                hipLaunchKernelGGL(fragfile_order_kernel, dim3(grid), dim3(kThreads), 0, stream, (const int32_t *)start_out_dev,
                                   (const uint32_t *)status_out_dev, (long long)n_lines, tracks, first_error);
                ROCCO_HIP_TRY(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(fragfile_report_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long *)first_error, (long long *)(sc + at.back));
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(back, sc + at.back, sizeof(back), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the one wait: the report, the staged arrays may go, the kernels' error state)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (int q = 0; q < 4; ++q) {
        report_out_host[q] = back[q];
    }
    return ROCCO_HIP_OK;
}

namespace {

// the tracks of a count call as the kernels read them; false where a region or an offset is refused
bool stage_tracks(const int64_t *line_offsets_host, size_t K, const rocco_hip_fragfile_options *options, const rocco_hip_count_region *regions,
                  const int64_t *out_offsets, std::vector<FragTrack> &tracks, size_t *n_cells)
{
    tracks.resize(K);
    size_t cells = 0;
    for (size_t k = 0; k < K; ++k) {
        const rocco_hip_count_region &r = regions[k];
        if (r.step <= 0 || r.n_bins < 0 || r.start < 0 || r.end < r.start || out_offsets[k] < 0 || options[k].count_mode < 0 ||
            options[k].count_mode > ROCCO_FRAGFILE_MODE_CENTER || line_offsets_host[k + 1] - line_offsets_host[k] >= (int64_t)0x7fffffff) {
            return false;
        }
        tracks[k] = {(long long)cells, (long long)out_offsets[k], r.start, r.end, r.step, r.n_bins, options[k].count_mode,
                     options[k].one_read_per_bin != 0 ? 1 : 0};
        cells += (size_t)r.n_bins + 1;
    }
    *n_cells = cells;
    return true;
}

}  // namespace

size_t fragfile_count_scratch_bytes(size_t K, const rocco_hip_count_region *regions_host)
{
    size_t cells = 0;
    for (size_t k = 0; k < K; ++k) {
        cells += (size_t)(regions_host[k].n_bins > 0 ? regions_host[k].n_bins : 0) + 1;
    }
    return TracksLayout(K, cells).bytes;
}

int launch_fragfile_count_batch(const int32_t *start_dev, const int32_t *end_dev, const int32_t *weight_dev, const uint32_t *status_dev,
                                const int64_t *line_offsets_host, size_t K, const rocco_hip_fragfile_options *options_host,
                                const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host, float *out_dev,
                                int64_t *max_magnitude_out_host, void *scratch_dev, hipStream_t stream)
{
    std::vector<FragTrack> tracks;
    size_t n_cells = 0;
    if (!offsets_ascend(line_offsets_host, K) || !stage_tracks(line_offsets_host, K, options_host, regions_host, out_offsets_host, tracks, &n_cells)) {
        set_last_error("fragfile_count_batch: line_offsets_host must ascend; a region needs 0 <= start <= end, step > 0, n_bins >= 0; a mode 0..3; "
                       "a track fewer than 2^31 lines");
        return ROCCO_HIP_EINVAL;
    }
    const TracksLayout at(K, n_cells);
    std::vector<char> staged(at.uploaded, 0);
    memcpy(staged.data() + at.line_first, line_offsets_host, (K + 1) * sizeof(int64_t));
    memcpy(staged.data() + at.tracks, tracks.data(), K * sizeof(FragTrack));
    char *sc = (char *)scratch_dev;
    unsigned long long *P = (unsigned long long *)(sc + at.cells), *N = P + n_cells;
    std::vector<long long> maxima(K, 0);
    const long long n_lines = line_offsets_host[K] - line_offsets_host[0];
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemcpyAsync(sc, staged.data(), staged.size(), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(sc + at.cells, 0, at.bytes - at.cells, stream));
        const FragTrack *tracks_dev = (const FragTrack *)(sc + at.tracks);
        if (n_lines > 0) {
            hipLaunchKernelGGL(fragfile_count_kernel, dim3(capped_grid((n_lines + kThreads - 1) / kThreads, ROCCO_FRAGFILE_COUNT_MAX_GRID)),
                               dim3(kThreads), 0, stream, start_dev, end_dev, weight_dev, status_dev, (const int64_t *)(sc + at.line_first), tracks_dev,
                               (long long)K, P, N);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(fragfile_finish_kernel, dim3(capped_grid((long long)K, ROCCO_FRAGFILE_COUNT_MAX_GRID)), dim3(kThreads), 0, stream,
                           tracks_dev, (long long)K, (const unsigned long long *)P, (const unsigned long long *)N, out_dev,
                           (long long *)(sc + at.maxima));
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(maxima.data(), sc + at.maxima, K * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the one wait: the magnitudes the caller judges the result by)
        ROCCO_HIP_TRY(hipGetLastError());
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

size_t fragfile_range_scratch_bytes(size_t K) { return TracksLayout(K, 0).bytes; }

int launch_fragfile_chrom_range_batch(const int32_t *start_dev, const int32_t *end_dev, const uint32_t *status_dev, const int64_t *line_offsets_host,
                                      const int64_t *chrom_len_host, size_t K, int64_t *range_out_host, void *scratch_dev, hipStream_t stream)
{
    if (!offsets_ascend(line_offsets_host, K)) {
        set_last_error("fragfile_chrom_range_batch: line_offsets_host must ascend from a non-negative begin");
        return ROCCO_HIP_EINVAL;
    }
    const TracksLayout at(K, 0);
    std::vector<char> staged(at.uploaded, 0);
    memcpy(staged.data() + at.line_first, line_offsets_host, (K + 1) * sizeof(int64_t));
    memcpy(staged.data() + at.tracks, chrom_len_host, K * sizeof(int64_t));
    char *sc = (char *)scratch_dev;
    unsigned long long *first = (unsigned long long *)(sc + at.first), *last = (unsigned long long *)(sc + at.last);
    std::vector<long long> range(2 * K, 0);
    const long long n_lines = line_offsets_host[K] - line_offsets_host[0];
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemcpyAsync(sc, staged.data(), staged.size(), hipMemcpyHostToDevice, stream));
        ROCCO_HIP_TRY(hipMemsetAsync(first, 0xff, K * sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(last, 0, K * sizeof(unsigned long long), stream));
        if (n_lines > 0) {
            hipLaunchKernelGGL(fragfile_range_kernel, dim3(capped_grid((n_lines + kThreads - 1) / kThreads, ROCCO_FRAGFILE_COUNT_MAX_GRID)),
                               dim3(kThreads), 0, stream, start_dev, end_dev, status_dev, (const int64_t *)(sc + at.line_first),
                               (const int64_t *)(sc + at.tracks), (long long)K, first, last);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(fragfile_range_fetch_kernel, dim3((unsigned)((K + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, start_dev, end_dev,
                           (long long)K, (const unsigned long long *)first, (const unsigned long long *)last, (long long *)(sc + at.maxima));
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(range.data(), sc + at.maxima, 2 * K * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the one wait; the staged arrays may go)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t q = 0; q < 2 * K; ++q) {
        range_out_host[q] = range[q];
    }
    return ROCCO_HIP_OK;
}

int launch_fragfile_mapped_count(const int32_t *weight_dev, const int32_t *name_dev, const uint32_t *status_dev, size_t n_lines, int count_mode,
                                 int one_read_per_bin, uint64_t *sum_out_host, void *scratch_dev, hipStream_t stream)
{
    unsigned long long *sum = (unsigned long long *)scratch_dev, back = 0;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(sum, 0, sizeof(unsigned long long), stream));
        if (n_lines > 0) {
            hipLaunchKernelGGL(fragfile_mapped_kernel, dim3(capped_grid((long long)((n_lines + kThreads - 1) / kThreads), ROCCO_FRAGFILE_COUNT_MAX_GRID)),
                               dim3(kThreads), 0, stream, weight_dev, name_dev, status_dev, (long long)n_lines, count_mode, one_read_per_bin, sum);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(&back, sum, sizeof(back), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    *sum_out_host = (uint64_t)back;
    return ROCCO_HIP_OK;
}

}  // namespace rocco
