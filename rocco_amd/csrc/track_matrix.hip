// rocco_amd/csrc/track_matrix.hip -- K count buffers -> the K' x m matrix of generate_chrom_matrix (DESIGN.md section 0 row
// f9), gfx950.
//
// Replaces the tail of get_bam_chrom_reads per file (rocco/readtracks.py:492-518: scale, trim to the positive support,
// np.round) together with the assembly of generate_chrom_matrix (rocco/readtracks.py:601-633: union of the starts, zeros,
// searchsorted, scatter, the float32 cast of low_memory) by one pass that writes every element of the matrix exactly once.
//
// Every track's count window starts at a multiple of step, so all tracks lie on one grid: bin i of a track whose window
// starts at count_start is grid index count_start / step + i.  The host merges the K' supports into at most K' disjoint,
// ascending segments of grid indices (a row of `segs`: the grid index and the column of the segment's first bin); the
// columns of the matrix are the segments laid end to end, which is np.unique(np.concatenate(starts)).  A thread bisects
// the segments for the first column of a 16-byte word and walks on from there; inside the row's support the value is
// np.round(tail(count), digits), outside it is +0.0.  Nothing is zeroed beforehand and nothing is scattered.
#include "count_tail.h"
#include "kernels.h"
#include "record_stream.h"
#include "round_np.h"

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_TRACK_MATRIX_THREADS;
constexpr int kUnit = ROCCO_TRACK_MATRIX_UNIT;     // columns of one row a workgroup writes at a time
constexpr int kMaxGrid = ROCCO_TRACK_MATRIX_MAX_GRID;
constexpr int kRowWords = ROCCO_TRACK_MATRIX_ROW_WORDS;

static_assert(kUnit % (kThreads * 4) == 0 && kThreads % 64 == 0 && kMaxGrid > 0 && kRowWords == 6, "rocco_hip.h states the shape");

template <typename T>
struct alignas(16) Pack {
    T v[16 / sizeof(T)];
};

// rows: int64 [n_rows][6] = offset of the track's counts in `counts`, its bins, the grid index of its bin 0, the grid
// indices of the first and the last bin of its support, its norm_scale (the float64's bits).  segs: int64 [n_segs][2].
// A row start is aligned to sizeof(T) only (m is arbitrary).  With a = the elements by which the row starts behind a
// 16-byte boundary, 16-byte word q of the row holds the columns q * kWord - a .. + kWord - 1; a unit is kUnit / kWord
// words, and in each of its passes the kThreads lanes take kThreads neighbouring words: a wavefront stores 1 KB in one
// piece and reads its counts from one stretch.  A word whose columns all exist is stored whole; the first and the last
// word of a row are stored one element at a time, what exists of them.
template <typename T>
__global__ __launch_bounds__(kThreads) void track_matrix_fill_kernel(const float *__restrict__ counts, long long counts_len,
                                                                    const long long *__restrict__ rows, int n_rows,
                                                                    const long long *__restrict__ segs, int n_segs, long long m,
                                                                    int units_per_row, int total_units, int scale_by_step,
                                                                    double step, double const_scale, int apply_const, double pow10,
                                                                    int digits, T *__restrict__ out)
{
    constexpr int kWord = 16 / sizeof(T);           // elements of one 16-byte store
    constexpr int kPasses = kUnit / kWord / kThreads;
    for (int unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
        const int row = unit / units_per_row, u = unit - row * units_per_row;
        const long long *__restrict__ r = rows + (long long)row * kRowWords;
        const long long counts_offset = r[0], n_bins = r[1], origin = r[2], g_first = r[3], g_last = r[4];
        const double norm_scale = __longlong_as_double(r[5]);
        T *__restrict__ row_out = out + (long long)row * m;
        const int a = (int)(((unsigned long long)row_out / sizeof(T)) & (kWord - 1));
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const long long j0 = ((long long)u * (kUnit / kWord) + pass * kThreads + threadIdx.x) * kWord - a;
            if (j0 >= m) {
                continue;  // (no barrier in this loop)
            }
            const long long jf = j0 < 0 ? 0 : j0;
            int s = 0;
            {  // largest s with segs[2 s + 1] <= jf (segs[1] is 0)
                int hi = n_segs;
                while (hi - s > 1) {
                    const int mid = (s + hi) >> 1;
                    if (segs[2 * mid + 1] <= jf) {
                        s = mid;
                    } else {
                        hi = mid;
                    }
                }
            }
            long long g = segs[2 * s] + (jf - segs[2 * s + 1]);
            long long next_col = s + 1 < n_segs ? segs[2 * (s + 1) + 1] : m;
            Pack<T> p;
#pragma unroll
            for (int i = 0; i < kWord; ++i) {
                const long long j = j0 + i;
                p.v[i] = (T)0;
                if (j < 0 || j >= m) {
                    continue;
                }
                if (j >= next_col && s + 1 < n_segs) {  // the next segment begins at this column
                    ++s;
                    g = segs[2 * s];
                    next_col = s + 1 < n_segs ? segs[2 * (s + 1) + 1] : m;
                }
                const long long bin = g - origin;
                if (g >= g_first && g <= g_last && bin >= 0 && bin < n_bins && counts_offset >= 0 && counts_offset + bin < counts_len) {
                    const double scaled = count_tail_value(counts[counts_offset + bin], norm_scale, scale_by_step, step, apply_const, const_scale);
                    p.v[i] = (T)round_like_numpy(scaled, pow10, digits);  // (float32: round to nearest even, as NumPy casts)
                }
                ++g;
            }
            if (j0 >= 0 && j0 + kWord <= m) {
                *reinterpret_cast<Pack<T> *>(row_out + j0) = p;
            } else {
#pragma unroll
                for (int i = 0; i < kWord; ++i) {
                    if (j0 + i >= 0 && j0 + i < m) {
                        row_out[j0 + i] = p.v[i];
                    }
                }
            }
        }
    }
}

}  // namespace

int launch_track_matrix_fill(const float *counts_dev, size_t counts_len, const int64_t *rows_dev, size_t n_rows, const int64_t *segs_dev,
                             size_t n_segs, size_t m, int scale_by_step, double step, double const_scale, int round_digits,
                             int out_dtype, void *matrix_out_dev, hipStream_t stream)
{
    const long long word = out_dtype == 0 ? 2 : 4;  // elements of a 16-byte store
    const long long units_per_row = ((long long)m + (word - 1) + kUnit - 1) / kUnit;
    const long long total_units = units_per_row * (long long)n_rows;
    if (total_units >= (1LL << 31) - kMaxGrid) {  // (the kernel counts units in an int, a grid stride past the last included)
        set_last_error("track_matrix_fill: the matrix has too many elements for one call");
        return ROCCO_HIP_EINVAL;
    }
    const unsigned grid = (unsigned)(total_units < (long long)kMaxGrid ? total_units : (long long)kMaxGrid);
    const int apply_const = const_scale >= 0.0 ? 1 : 0;
    if (out_dtype == 0) {
        hipLaunchKernelGGL(track_matrix_fill_kernel<double>, dim3(grid), dim3(kThreads), 0, stream, counts_dev, (long long)counts_len,
                           (const long long *)rows_dev, (int)n_rows, (const long long *)segs_dev, (int)n_segs, (long long)m,
                           (int)units_per_row, (int)total_units, scale_by_step, step, const_scale, apply_const, numpy_pow10(round_digits),
                           round_digits, (double *)matrix_out_dev);
    } else {
        hipLaunchKernelGGL(track_matrix_fill_kernel<float>, dim3(grid), dim3(kThreads), 0, stream, counts_dev, (long long)counts_len,
                           (const long long *)rows_dev, (int)n_rows, (const long long *)segs_dev, (int)n_segs, (long long)m,
                           (int)units_per_row, (int)total_units, scale_by_step, step, const_scale, apply_const, numpy_pow10(round_digits),
                           round_digits, (float *)matrix_out_dev);
    }
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;  // (no wait: the tables are the caller's device arrays, nothing here lives in the solver's scratch)
}

}  // namespace rocco
