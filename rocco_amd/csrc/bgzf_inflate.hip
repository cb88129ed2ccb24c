// rocco_amd/csrc/bgzf_inflate.hip -- the BGZF blocks of a BAM file -> their inflated bytes, checked against ISIZE and CRC32
// (note (29)), gfx950.
//
// Replaces what the reference has htslib's BGZF reader do per block (bgzf_read_block: inflate, the length and the CRC32 of the
// trailer).  A file is thousands of independent DEFLATE streams of at most 64 KiB: the parallelism is across blocks, inside a
// block the Huffman decode is one dependent chain.  So one wavefront takes one block (a workgroup IS one wavefront: no
// communication between workgroups, no waiting on another); all 64 lanes carry the same decoder state, the code tables are
// built by the lanes together into LDS, and the bytes of a match or of a stored block are copied by the lanes side by side
// (inflate_core.h, which states the rules once for this file and for the host).
//
// The output goes straight to HBM and a match reads it back from there; there is no 64 KiB window in LDS.  Reason: the
// dependent chain of one wavefront leaves its SIMD idle most of the time, and only other wavefronts fill it.  A 64 KiB window
// admits 2 wavefronts per CU (160 KiB of LDS), the 6 KiB of tables and staging used here admit 24 or more.  The price is that
// the stores of the wavefront must have drained before a match loads what they wrote: x.sync() does that (workgroup-scope
// release/acquire, i.e. a wait for the outstanding stores), and inflate_block asks for it only when a match reaches into bytes
// written since the last one.  Neither layout has been measured against the other.
#include "kernels.h"
#include "inflate_core.h"
#include "record_layouts.h"

namespace rocco {

namespace {

constexpr int kWave = ROCCO_BGZF_THREADS;
constexpr int kStage = 512;  // bytes of the compressed span kept in LDS in front of the bit reader
constexpr long long kMaxGrid = ROCCO_BGZF_MAX_GRID;  // workgroups of a launch at most: a later block is a workgroup's next turn

static_assert(kWave == 64 && kCrcChunks == kWave, "one lane per CRC chunk; rocco_hip.h states the shape");

struct DeviceInflateExec {
    static constexpr int kLanes = kWave;
    const uint8_t *comp;
    long long hi;           // loads stay below it
    uint8_t *stage;         // LDS
    long long stage_first;  // stage[k] = comp[stage_first + k]
    int lane_;

    __device__ int lane() const { return lane_; }
    __device__ uint64_t ballot(bool p) const { return __ballot(p); }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint8_t in_raw(long long i) const { return comp[i]; }
    __device__ uint32_t in_byte(long long i)
    {
        if (i < stage_first || i >= stage_first + kStage) {  // (the same i in every lane)
            __syncthreads();
            stage_first = i;
            for (int k = lane_; k < kStage; k += kWave) {
                stage[k] = i + k < hi ? comp[i + k] : (uint8_t)0;
            }
            __syncthreads();
        }
        return stage[i - stage_first];
    }
};

struct DeviceCrcExec {
    static constexpr int kLanes = kWave;
    int lane_;
    __device__ int lane() const { return lane_; }
    __device__ void sync() const { __syncthreads(); }
};

__device__ __forceinline__ void note_first(unsigned long long *first_error, long long block, int status)
{
    atomicMin(first_error, ((unsigned long long)block << 32) | (unsigned long long)(unsigned)status);
}

// one wavefront per block (grid stride).  status[i]: 0, ROCCO_BGZF_ERR_STREAM | why << 8, _LENGTH or _TABLE; produced[i]: the
// bytes the stream inflates to; first_error: the lowest (block << 32 | status) of a failing block
__global__ __launch_bounds__(kWave) void bgzf_inflate_kernel(const uint8_t *__restrict__ comp, long long n_comp,
                                                            const int64_t *__restrict__ table, long long n_blocks, uint8_t *out,
                                                            long long n_out, int *__restrict__ status, long long *__restrict__ produced,
                                                            unsigned long long *__restrict__ first_error)
{
    __shared__ InflateTables tables;
    __shared__ uint8_t stage[kStage];
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        int64_t row[ROCCO_BGZF_TABLE_COLUMNS];
        for (int k = 0; k < ROCCO_BGZF_TABLE_COLUMNS; ++k) {
            row[k] = table[i * ROCCO_BGZF_TABLE_COLUMNS + k];
        }
        int result = ROCCO_BGZF_ERR_TABLE;
        long long made = 0;
        if (bgzf_row_fits(row, n_comp, n_out)) {
            // (stage_first = hi: no byte of the span is staged yet)
            DeviceInflateExec x = {comp, row[1], stage, row[1], (int)threadIdx.x};
            result = inflate_block(x, tables, row[0], row[1], out + row[4], row[2], &made);
        }
        if (threadIdx.x == 0) {
            status[i] = result;
            produced[i] = made;
            if (result != 0) {
                note_first(first_error, i, result);
            }
        }
    }
}

// one wavefront per block that inflated: lane c takes chunk c of its bytes, the 64 CRCs are combined pairwise
__global__ __launch_bounds__(kWave) void bgzf_crc_kernel(const int64_t *__restrict__ table, long long n_blocks,
                                                        const uint8_t *__restrict__ out, int *__restrict__ status,
                                                        unsigned long long *__restrict__ first_error)
{
    __shared__ CrcTables tables;
    const int lane = threadIdx.x;
    DeviceCrcExec x = {lane};
    crc_tables_build(x, tables);
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        if (status[i] != 0) {  // (a row that does not fit is among them: nothing of it is read)
            continue;
        }
        const int64_t *row = table + i * ROCCO_BGZF_TABLE_COLUMNS;
        long long first, length;
        crc_chunk(row[2], lane, &first, &length);
        uint32_t crc = crc_of_bytes(tables, out + row[4] + first, length);
        for (int step = 1; step < kWave; step <<= 1) {
            const uint32_t crc_right = __shfl_down(crc, step);
            const long long length_right = __shfl_down(length, step);
            if ((lane & (2 * step - 1)) == 0) {
                crc = crc_combine(tables, crc, crc_right, length_right);
                length += length_right;
            }
        }
        if (lane == 0 && crc != (uint32_t)row[3]) {
            status[i] = ROCCO_BGZF_ERR_CRC;
            note_first(first_error, i, ROCCO_BGZF_ERR_CRC);
        }
    }
}

// report: [0] the first failing block or -1, [1] its status, [2] the bytes it inflates to
__global__ void bgzf_report_kernel(const unsigned long long *__restrict__ first_error, const long long *__restrict__ produced,
                                   long long *__restrict__ report)
{
    const unsigned long long packed = *first_error;
    const bool none = packed == ~0ULL;
    report[0] = none ? -1 : (long long)(packed >> 32);
    report[1] = none ? 0 : (long long)(packed & 0xffffffffULL);
    report[2] = none ? 0 : produced[packed >> 32];
    report[3] = 0;
}

// ---- zlib framing: the data blocks of a bigWig file (note (31)) ------------------------------------------
constexpr long long kZlibMaxGrid = ROCCO_ZLIB_MAX_GRID;

// one wavefront per block (grid stride): the header, the stream, the room for the check value, the length; a stored row is
// copied.  status[i] == 0 with framing 0: the Adler-32 is still to be compared, at comp[ends[i]]
__global__ __launch_bounds__(kWave) void zlib_inflate_kernel(const uint8_t *__restrict__ comp, long long n_comp,
                                                            const int64_t *__restrict__ table, long long n_blocks, uint8_t *out,
                                                            long long n_out, int *__restrict__ status, long long *__restrict__ produced,
                                                            long long *__restrict__ ends, unsigned long long *__restrict__ first_error)
{
    __shared__ InflateTables tables;
    __shared__ uint8_t stage[kStage];
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        int64_t row[ROCCO_ZLIB_TABLE_COLUMNS];
        for (int k = 0; k < ROCCO_ZLIB_TABLE_COLUMNS; ++k) {
            row[k] = table[i * ROCCO_ZLIB_TABLE_COLUMNS + k];
        }
        int result = ROCCO_BGZF_ERR_TABLE;
        long long made = 0, end = 0;
        if (zlib_row_fits(row, n_comp, n_out)) {
            DeviceInflateExec x = {comp, row[1], stage, row[1], (int)threadIdx.x};
            result = zlib_block(x, tables, row, out + row[3], &made, &end);
        }
        if (threadIdx.x == 0) {
            status[i] = result;
            produced[i] = made;
            ends[i] = end;
            if (result != 0) {
                note_first(first_error, i, result);
            }
        }
    }
}

// one wavefront per sound zlib block: lane c takes chunk c of its produced bytes, the 64 Adler-32s are combined pairwise
__global__ __launch_bounds__(kWave) void zlib_adler_kernel(const uint8_t *__restrict__ comp, const int64_t *__restrict__ table,
                                                          long long n_blocks, const uint8_t *__restrict__ out, int *__restrict__ status,
                                                          const long long *__restrict__ produced, const long long *__restrict__ ends,
                                                          unsigned long long *__restrict__ first_error)
{
    const int lane = threadIdx.x;
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        const int64_t *row = table + i * ROCCO_ZLIB_TABLE_COLUMNS;
        if (status[i] != 0 || row[4] != 0) {  // (a row that does not fit is among them: nothing of it is read)
            continue;
        }
        long long first, length;
        crc_chunk(produced[i], lane, &first, &length);  // (status 0: produced <= capacity, the chunk lies in the slot)
        uint32_t adler = adler_of_bytes(out + row[3] + first, length);
        for (int step = 1; step < kWave; step <<= 1) {
            const uint32_t adler_right = __shfl_down(adler, step);
            const long long length_right = __shfl_down(length, step);
            if ((lane & (2 * step - 1)) == 0) {
                adler = adler_combine(adler, adler_right, length_right);
                length += length_right;
            }
        }
        if (lane == 0 && adler != zlib_stated_adler(comp, ends[i])) {  // (status 0: ends + 4 <= the span's end)
            status[i] = ROCCO_ZLIB_ERR_ADLER;
            note_first(first_error, i, ROCCO_ZLIB_ERR_ADLER);
        }
    }
}

}  // namespace

size_t zlib_inflate_scratch_bytes(size_t n_blocks) { return ZlibInflateLayout(n_blocks).bytes; }

int launch_zlib_inflate(const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks, uint8_t *out_dev, size_t n_out,
                        int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    const ZlibInflateLayout at(n_blocks);
    char *sc = (char *)scratch_dev;
    int *status = status_out_dev != nullptr ? status_out_dev : (int *)(sc + at.status);
    long long *produced = produced_out_dev != nullptr ? (long long *)produced_out_dev : (long long *)(sc + at.produced);
    long long *ends = (long long *)(sc + at.ends), *report = (long long *)(sc + at.report);
    unsigned long long *first_error = (unsigned long long *)(sc + at.first_error);
    long long back[ROCCO_BGZF_REPORT] = {-1, 0, 0, 0};
    if (n_blocks > 0) {
        const unsigned grid = (unsigned)((long long)n_blocks < kZlibMaxGrid ? (long long)n_blocks : kZlibMaxGrid);
        const int queued = queue_then_drain(stream, [&]() -> int {
            ROCCO_HIP_TRY(hipMemsetAsync(first_error, 0xff, sizeof(unsigned long long), stream));
            hipLaunchKernelGGL(zlib_inflate_kernel, dim3(grid), dim3(kWave), 0, stream, comp_dev, (long long)n_comp, table_dev,
                               (long long)n_blocks, out_dev, (long long)n_out, status, produced, ends, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(zlib_adler_kernel, dim3(grid), dim3(kWave), 0, stream, comp_dev, table_dev, (long long)n_blocks,
                               (const uint8_t *)out_dev, status, (const long long *)produced, (const long long *)ends, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bgzf_report_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long *)first_error,
                               (const long long *)produced, report);
            ROCCO_HIP_TRY(hipGetLastError());
            ROCCO_HIP_TRY(hipMemcpyAsync(back, report, sizeof(back), hipMemcpyDeviceToHost, stream));
            ROCCO_HIP_TRY(hipStreamSynchronize(stream));
            return ROCCO_HIP_OK;
        });
        if (queued != ROCCO_HIP_OK) {
            return queued;
        }
    }
    for (int k = 0; k < ROCCO_BGZF_REPORT; ++k) {
        report_out_host[k] = back[k];
    }
    return ROCCO_HIP_OK;
}

void zlib_inflate_host_blocks(const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks, uint8_t *out, size_t n_out,
                              int32_t *status_out, int64_t *produced_out, int64_t *report_out)
{
    zlib_inflate_host(comp, (long long)n_comp, table, (long long)n_blocks, out, (long long)n_out, status_out, produced_out, report_out);
    report_out[3] = 0;
}

size_t bgzf_inflate_scratch_bytes(size_t n_blocks) { return BgzfInflateLayout(n_blocks).bytes; }

int launch_bgzf_inflate(const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks, uint8_t *out_dev, size_t n_out,
                        int32_t *status_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    const BgzfInflateLayout at(n_blocks);
    char *sc = (char *)scratch_dev;
    int *status = status_out_dev != nullptr ? status_out_dev : (int *)(sc + at.status);
    long long *produced = (long long *)(sc + at.produced), *report = (long long *)(sc + at.report);
    unsigned long long *first_error = (unsigned long long *)(sc + at.first_error);
    long long back[ROCCO_BGZF_REPORT] = {-1, 0, 0, 0};
    if (n_blocks > 0) {
        const unsigned grid = (unsigned)((long long)n_blocks < kMaxGrid ? (long long)n_blocks : kMaxGrid);
        const int queued = queue_then_drain(stream, [&]() -> int {
            ROCCO_HIP_TRY(hipMemsetAsync(first_error, 0xff, sizeof(unsigned long long), stream));
            hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(grid), dim3(kWave), 0, stream, comp_dev, (long long)n_comp, table_dev,
                               (long long)n_blocks, out_dev, (long long)n_out, status, produced, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bgzf_crc_kernel, dim3(grid), dim3(kWave), 0, stream, table_dev, (long long)n_blocks, (const uint8_t *)out_dev,
                               status, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bgzf_report_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long *)first_error,
                               (const long long *)produced, report);
            ROCCO_HIP_TRY(hipGetLastError());
            ROCCO_HIP_TRY(hipMemcpyAsync(back, report, sizeof(back), hipMemcpyDeviceToHost, stream));
            ROCCO_HIP_TRY(hipStreamSynchronize(stream));
            return ROCCO_HIP_OK;
        });
        if (queued != ROCCO_HIP_OK) {
            return queued;
        }
    }
    for (int k = 0; k < ROCCO_BGZF_REPORT; ++k) {
        report_out_host[k] = back[k];
    }
    return ROCCO_HIP_OK;
}

void bgzf_inflate_host_blocks(const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks, uint8_t *out, size_t n_out,
                              int32_t *status_out, int64_t *report_out)
{
    bgzf_inflate_host(comp, (long long)n_comp, table, (long long)n_blocks, out, (long long)n_out, status_out, report_out);
    report_out[3] = 0;
}

}  // namespace rocco
