// rocco_amd/csrc/bigwig_sections.hip -- the inflated data sections of bigWig files -> (starts, ends, values) in HBM, gfx950
// (note (31)).  The rules are bigwig_sections.h's, the same source the host twin compiles.
//
// Two calls.  facts: one wavefront per block (a grid stride under ROCCO_BIGWIG_MAX_GRID) judges the row, the header and the
// items and counts the kept ones with ballots; hipcub's exclusive sum over the n + 1 counts gives every block's first output
// index; a tail kernel gathers the files' interval offsets and the report; ONE wait brings them back, and with it the error
// state of these kernels.  emit: one wavefront per block repeats the item walk and places each kept item by its ballot prefix
// within the 64-item turn, between its block's first index and the least of the next block's and the arrays' capacity.
// Bound: the sections' bytes read once per call, 24 bytes written per kept item.  No LDS, no scratch memory.
#include <hipcub/hipcub.hpp>

#include "bigwig_sections.h"
#include "kernels.h"
#include "record_layouts.h"

namespace rocco {

namespace {

constexpr int kWave = ROCCO_BIGWIG_THREADS;

struct DeviceSectionExec {
    static constexpr int kLanes = kWave;
    int lane_;
    __device__ int lane() const { return lane_; }
    __device__ unsigned long long ballot(bool on) const { return __ballot(on); }
    __device__ static int bits(unsigned long long mask) { return __popcll(mask); }
};

// what the kernels know of the files: file_first [n_files + 1], then chrom_id [n_files], then chrom_length [n_files]
struct SectionFiles {
    const long long *first, *chrom_id, *chrom_length;
    long long n;
};

__global__ __launch_bounds__(kWave) void sections_facts_kernel(const uint8_t *__restrict__ slots, long long n_slots,
                                                              const int64_t *__restrict__ table, const int64_t *__restrict__ produced,
                                                              long long n_blocks, SectionFiles files, int *__restrict__ status,
                                                              long long *__restrict__ counts, unsigned long long *__restrict__ first_error)
{
    const DeviceSectionExec x = {(int)threadIdx.x};
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        int64_t row[ROCCO_ZLIB_TABLE_COLUMNS];
        for (int c = 0; c < ROCCO_ZLIB_TABLE_COLUMNS; ++c) {
            row[c] = table[i * ROCCO_ZLIB_TABLE_COLUMNS + c];
        }
        const long long k = section_file(files.first, files.n, i);
        long long kept = 0;
        const int result = section_facts(x, slots, n_slots, row, produced[i], files.chrom_id[k], files.chrom_length[k], &kept);
        if (threadIdx.x == 0) {
            status[i] = result;
            counts[i] = kept;
            if (result != 0) {
                atomicMin(first_error, ((unsigned long long)i << 32) | (unsigned long long)(unsigned)result);
            }
        }
    }
}

// back: [0 .. ROCCO_BGZF_REPORT) the report (first refused block or -1, its status, the kept items of all blocks, 0), then the
// n_files + 1 interval offsets of the files
__global__ void sections_tail_kernel(const unsigned long long *__restrict__ first_error, const long long *__restrict__ block_first,
                                     long long n_blocks, SectionFiles files, long long *__restrict__ back)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= files.n) {
        back[ROCCO_BGZF_REPORT + t] = block_first[files.first[t]];
    }
    if (t == 0) {
        const unsigned long long packed = *first_error;
        const bool none = packed == ~0ULL;
        back[0] = none ? -1 : (long long)(packed >> 32);
        back[1] = none ? 0 : (long long)(packed & 0xffffffffULL);
        back[2] = block_first[n_blocks];
        back[3] = 0;
    }
}

__global__ __launch_bounds__(kWave) void sections_emit_kernel(const uint8_t *__restrict__ slots, long long n_slots,
                                                             const int64_t *__restrict__ table, const int64_t *__restrict__ produced,
                                                             long long n_blocks, SectionFiles files, const long long *__restrict__ block_first,
                                                             long long capacity, int64_t *__restrict__ starts, int64_t *__restrict__ ends,
                                                             uint64_t *__restrict__ values)
{
    const DeviceSectionExec x = {(int)threadIdx.x};
    for (long long i = blockIdx.x; i < n_blocks; i += gridDim.x) {
        const long long first = block_first[i], next = block_first[i + 1];
        const long long limit = next < capacity ? next : capacity;
        if (first < 0 || first >= limit) {  // (nothing kept, or indices that are not this call's: nothing is written)
            continue;
        }
        int64_t row[ROCCO_ZLIB_TABLE_COLUMNS];
        for (int c = 0; c < ROCCO_ZLIB_TABLE_COLUMNS; ++c) {
            row[c] = table[i * ROCCO_ZLIB_TABLE_COLUMNS + c];
        }
        const long long made = produced[i];
        if (!section_fits(row, made, n_slots)) {
            continue;
        }
        const long long k = section_file(files.first, files.n, i);
        SectionHeader h;
        bool skip;
        if (section_judge(slots + row[3], made, files.chrom_id[k], &h, &skip) != 0 || skip) {
            continue;
        }
        section_emit(x, slots + row[3], h, files.chrom_length[k], first, limit, starts, ends, values);
    }
}

size_t sections_scan_bytes(size_t n_blocks)
{
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const long long *)nullptr, (long long *)nullptr, (int)(n_blocks + 1)) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes > 0 ? bytes : 1;
}

unsigned sections_grid(size_t n_blocks)
{
    return (unsigned)(n_blocks < (size_t)ROCCO_BIGWIG_MAX_GRID ? n_blocks : (size_t)ROCCO_BIGWIG_MAX_GRID);
}

// the three file arrays, one behind the other, queued to `files_dev`
int upload_files(const int64_t *file_first_host, const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                 long long *files_dev, std::vector<long long> &staged, hipStream_t stream, SectionFiles *files)
{
    staged.assign(file_first_host, file_first_host + n_files + 1);
    staged.insert(staged.end(), chrom_id_host, chrom_id_host + n_files);
    staged.insert(staged.end(), chrom_length_host, chrom_length_host + n_files);
    ROCCO_HIP_TRY(hipMemcpyAsync(files_dev, staged.data(), staged.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    *files = {files_dev, files_dev + n_files + 1, files_dev + 2 * n_files + 1, (long long)n_files};
    return ROCCO_HIP_OK;
}

}  // namespace

size_t bigwig_sections_scratch_bytes(size_t n_blocks, size_t n_files)
{
    const size_t scan = sections_scan_bytes(n_blocks);
    return scan == 0 ? 0 : SectionsLayout(n_blocks, n_files, scan).bytes;
}

int launch_bigwig_sections_facts(const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev, const int64_t *produced_dev, size_t n_blocks,
                                 const int64_t *file_first_host, const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                 int32_t *status_out_dev, int64_t *block_first_out_dev, int64_t *file_offsets_out_host, int64_t *report_out_host,
                                 void *scratch_dev, hipStream_t stream)
{
    const SectionsLayout at(n_blocks, n_files, sections_scan_bytes(n_blocks));
    char *sc = (char *)scratch_dev;
    long long *counts = (long long *)(sc + at.counts), *back_dev = (long long *)(sc + at.back);
    unsigned long long *first_error = (unsigned long long *)(sc + at.first_error);
    size_t scan_bytes = at.bytes - at.scan;
    std::vector<long long> staged, back(ROCCO_BGZF_REPORT + n_files + 1, 0);
    const int queued = queue_then_drain(stream, [&]() -> int {
        SectionFiles files;
        if (const int rc = upload_files(file_first_host, chrom_id_host, chrom_length_host, n_files, (long long *)(sc + at.files), staged, stream, &files);
            rc != ROCCO_HIP_OK) {
            return rc;
        }
        ROCCO_HIP_TRY(hipMemsetAsync(first_error, 0xff, sizeof(unsigned long long), stream));
        ROCCO_HIP_TRY(hipMemsetAsync(counts + n_blocks, 0, sizeof(long long), stream));
        if (n_blocks > 0) {
            hipLaunchKernelGGL(sections_facts_kernel, dim3(sections_grid(n_blocks)), dim3(kWave), 0, stream, slots_dev, (long long)n_slots,
                               table_dev, produced_dev, (long long)n_blocks, files, status_out_dev, counts, first_error);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const long long *)counts, (long long *)block_first_out_dev,
                                                       (int)(n_blocks + 1), stream));
        hipLaunchKernelGGL(sections_tail_kernel, dim3((unsigned)((n_files + 1 + 255) / 256)), dim3(256), 0, stream,
                           (const unsigned long long *)first_error, (const long long *)block_first_out_dev, (long long)n_blocks, files, back_dev);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(back.data(), back_dev, back.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the one wait: totals, report, and the error state of the kernels above)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (int k = 0; k < ROCCO_BGZF_REPORT; ++k) {
        report_out_host[k] = back[k];
    }
    for (size_t k = 0; k <= n_files; ++k) {
        file_offsets_out_host[k] = back[ROCCO_BGZF_REPORT + k];
    }
    return ROCCO_HIP_OK;
}

int launch_bigwig_sections_emit(const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev, const int64_t *produced_dev, size_t n_blocks,
                                const int64_t *file_first_host, const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                const int64_t *block_first_dev, size_t capacity, int64_t *starts_out_dev, int64_t *ends_out_dev,
                                double *values_out_dev, void *scratch_dev, hipStream_t stream)
{
    const SectionsLayout at(n_blocks, n_files, 1);
    char *sc = (char *)scratch_dev;
    std::vector<long long> staged;
    return queue_then_drain(stream, [&]() -> int {
        SectionFiles files;
        if (const int rc = upload_files(file_first_host, chrom_id_host, chrom_length_host, n_files, (long long *)(sc + at.files), staged, stream, &files);
            rc != ROCCO_HIP_OK) {
            return rc;
        }
        hipLaunchKernelGGL(sections_emit_kernel, dim3(sections_grid(n_blocks)), dim3(kWave), 0, stream, slots_dev, (long long)n_slots, table_dev,
                           produced_dev, (long long)n_blocks, files, (const long long *)block_first_dev, (long long)capacity, starts_out_dev,
                           ends_out_dev, (uint64_t *)values_out_dev);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));  // (the staged file arrays may go; a fault of this kernel is this call's error)
        ROCCO_HIP_TRY(hipGetLastError());
        return ROCCO_HIP_OK;
    });
}

}  // namespace rocco
