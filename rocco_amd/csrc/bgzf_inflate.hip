// rocco_amd/csrc/bgzf_inflate.hip -- a table of independent DEFLATE blocks -> their inflated bytes, each checked against its
// length and check value: the BGZF blocks of a BAM file (ISIZE and CRC32; DESIGN.md section 0 row f8, note (29)) and the
// zlib-framed data blocks of a bigWig file (capacity and Adler-32; row f10, note (31)), gfx950.
//
// ONE kernel pair, launcher and report for both: inflate_kernel<F>, check_kernel<F>, report_kernel and launch_inflate<F>, where
// the framing F (BgzfFraming, ZlibFraming of inflate_core.h) states at compile time what differs: the table's columns, the grid
// cap, what surrounds the deflate data, and the check.
//
// Replaces what the reference has htslib's BGZF reader do per block (bgzf_read_block: inflate, the length and the CRC32 of the
// trailer) and what libBigWig has zlib's uncompress() do per data block.  A file is thousands of independent DEFLATE streams of
// at most 64 KiB: the parallelism is across blocks, inside a block the Huffman decode is one dependent chain.  So one wavefront takes one block (a workgroup IS one wavefront: no
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

struct DeviceCheckExec {
    static constexpr int kLanes = kWave;
    int lane_;
    __device__ int lane() const { return lane_; }
    __device__ void sync() const { __syncthreads(); }
};

__device__ __forceinline__ void note_first(unsigned long long *first_error, long long block, int status)
{
    atomicMin(first_error, ((unsigned long long)block << 32) | (unsigned long long)(unsigned)status);
}

// what check_kernel reads besides the table and the inflated bytes: nothing where the row states the check value (BGZF), else
// the compressed buffer, and per block the bytes it produced and where its stream ended (zlib)
template <bool kStatedInStream>
struct CheckSource {
};
template <>
struct CheckSource<true> {
    const uint8_t *comp;
    const long long *produced, *ends;
};

// one wavefront per block (grid stride: a later block is a workgroup's next turn).  status[i]: 0 or why not, in the framing's
// codes (rocco_hip.h) -- 0 where the row has a check value: that is still to be compared; produced[i]: the bytes the stream
// inflates to; ends[i] (only where the check value stands in the stream): where it stands in comp; first_error: the lowest
// (block << 32 | status) of a failing block
template <class F>
__global__ __launch_bounds__(kWave) void inflate_kernel(const uint8_t *__restrict__ comp, long long n_comp, const int64_t *__restrict__ table,
                                                       long long n_blocks, uint8_t *out, long long n_out, int *__restrict__ status,
                                                       long long *__restrict__ produced, long long *__restrict__ ends,
                                                       unsigned long long *__restrict__ first_error)
{
    __shared__ InflateTables tables;
    __shared__ uint8_t stage[kStage];
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        int64_t row[F::kColumns];
        for (int k = 0; k < F::kColumns; ++k) {
            row[k] = table[i * F::kColumns + k];
        }
        int result = ROCCO_BGZF_ERR_TABLE;
        long long made = 0, end = 0;
        if (F::fits(row, n_comp, n_out)) {
            // (stage_first = hi: no byte of the span is staged yet)
            DeviceInflateExec x = {comp, row[1], stage, row[1], (int)threadIdx.x};
            result = F::block(x, tables, row, out + row[F::kOffsetColumn], &made, &end);
        }
        if (threadIdx.x == 0) {
            status[i] = result;
            produced[i] = made;
            if constexpr (F::kStatedInStream) {
                ends[i] = end;
            }
            if (result != 0) {
                note_first(first_error, i, result);
            }
        }
    }
}

// one wavefront per block that inflated and has a check value: lane c takes chunk c of the bytes it covers, the 64 values are
// combined pairwise
template <class F>
__global__ __launch_bounds__(kWave) void check_kernel(const int64_t *__restrict__ table, long long n_blocks, const uint8_t *__restrict__ out,
                                                     int *__restrict__ status, CheckSource<F::kStatedInStream> from,
                                                     unsigned long long *__restrict__ first_error)
{
    __shared__ typename F::CheckTables tables;  // (no LDS where the framing's are empty)
    const int lane = threadIdx.x;
    DeviceCheckExec x = {lane};
    F::check_tables_build(x, tables);
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        const int64_t *row = table + i * F::kColumns;
        if (status[i] != 0 || !F::has_check(row)) {  // (a row that does not fit is among them: nothing of it is read)
            continue;
        }
        long long covered = 0, end = 0;
        const uint8_t *comp = nullptr;
        if constexpr (F::kStatedInStream) {  // (status 0: produced <= capacity, the chunk lies in the slot; end + 4 <= the span's end)
            covered = from.produced[i];
            end = from.ends[i];
            comp = from.comp;
        }
        long long first, length;
        crc_chunk(F::check_bytes(row, covered), lane, &first, &length);
        uint32_t check = F::check_chunk(tables, out + row[F::kOffsetColumn] + first, length);
        for (int step = 1; step < kWave; step <<= 1) {
            const uint32_t check_right = __shfl_down(check, step);
            const long long length_right = __shfl_down(length, step);
            if ((lane & (2 * step - 1)) == 0) {
                check = F::check_combine(tables, check, check_right, length_right);
                length += length_right;
            }
        }
        if (lane == 0 && check != F::stated(row, comp, end)) {
            status[i] = F::kCheckError;
            note_first(first_error, i, F::kCheckError);
        }
    }
}

// report: [0] the first failing block or -1, [1] its status, [2] the bytes it inflates to
__global__ void report_kernel(const unsigned long long *__restrict__ first_error, const long long *__restrict__ produced,
                              long long *__restrict__ report)
{
    const unsigned long long packed = *first_error;
    const bool none = packed == ~0ULL;
    report[0] = none ? -1 : (long long)(packed >> 32);
    report[1] = none ? 0 : (long long)(packed & 0xffffffffULL);
    report[2] = none ? 0 : produced[packed >> 32];
    report[3] = 0;
}

}  // namespace

template <class F>
size_t inflate_scratch_bytes(size_t n_blocks)
{
    return InflateLayout(n_blocks, F::kStatedInStream).bytes;
}

template <class F>
int launch_inflate(const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks, uint8_t *out_dev, size_t n_out,
                   int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    const InflateLayout at(n_blocks, F::kStatedInStream);
    char *sc = (char *)scratch_dev;
    int *status = status_out_dev != nullptr ? status_out_dev : (int *)(sc + at.status);
    long long *produced = produced_out_dev != nullptr ? (long long *)produced_out_dev : (long long *)(sc + at.produced);
    long long *ends = F::kStatedInStream ? (long long *)(sc + at.ends) : nullptr, *report = (long long *)(sc + at.report);
    unsigned long long *first_error = (unsigned long long *)(sc + at.first_error);
    CheckSource<F::kStatedInStream> from;
    if constexpr (F::kStatedInStream) {
        from = {comp_dev, produced, ends};
    }
    long long back[ROCCO_BGZF_REPORT] = {-1, 0, 0, 0};
    if (n_blocks > 0) {
        const unsigned grid = (unsigned)((long long)n_blocks < F::kMaxGrid ? (long long)n_blocks : F::kMaxGrid);
        const int queued = queue_then_drain(stream, [&]() -> int {
            ROCCO_HIP_TRY(hipMemsetAsync(first_error, 0xff, sizeof(unsigned long long), stream));
            hipLaunchKernelGGL(inflate_kernel<F>, dim3(grid), dim3(kWave), 0, stream, comp_dev, (long long)n_comp, table_dev,
                               (long long)n_blocks, out_dev, (long long)n_out, status, produced, ends, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(check_kernel<F>, dim3(grid), dim3(kWave), 0, stream, table_dev, (long long)n_blocks, (const uint8_t *)out_dev,
                               status, from, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(report_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long *)first_error,
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

template size_t inflate_scratch_bytes<BgzfFraming>(size_t);
template size_t inflate_scratch_bytes<ZlibFraming>(size_t);
template int launch_inflate<BgzfFraming>(const uint8_t *, size_t, const int64_t *, size_t, uint8_t *, size_t, int32_t *, int64_t *, int64_t *,
                                         void *, hipStream_t);
template int launch_inflate<ZlibFraming>(const uint8_t *, size_t, const int64_t *, size_t, uint8_t *, size_t, int32_t *, int64_t *, int64_t *,
                                         void *, hipStream_t);

}  // namespace rocco
