// rocco_amd/csrc/select_network.h -- what the column kernels of median.hip and dispersion.hip share: the in-register
// Batcher network, the NaN test on the bit pattern and the workgroup order.  Both files are compiled with
// -fno-honor-nans (see the Makefile), so that the network is bare v_min_f64 / v_max_f64.
#pragma once

#include "common.h"

namespace rocco {
#if defined(__HIPCC__)

template <int N>
__device__ __forceinline__ void select_middle(double (&v)[N])
{
    // Batcher's merge exchange for arbitrary N; every index below is a compile-time constant
    // once the loops are fully unrolled.
#pragma unroll
    for (int p = 1; p < N; p <<= 1) {
#pragma unroll
        for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
            for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
                for (int i = 0; i <= ((k - 1 < N - j - k - 1) ? (k - 1) : (N - j - k - 1)); ++i) {
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const double a = v[i + j];
                        const double b = v[i + j + k];
                        v[i + j] = fmin(a, b);
                        v[i + j + k] = fmax(a, b);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ bool is_nan_bits(double x)
{
    // these files are compiled with -fno-honor-nans (so that the network is bare v_min_f64 / v_max_f64);
    // NaN tests therefore go through the bit pattern
    return (__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFLL) > 0x7FF0000000000000LL;
}

// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Rows are not aligned to
// cache lines (n is arbitrary), so neighbouring workgroups share the line that straddles their
// boundary in every row: give each XCD one contiguous range of loci so that the shared lines meet
// in one L2 instead of being fetched from memory twice.
__device__ __forceinline__ unsigned xcd_contiguous_block()
{
    const unsigned nblk = gridDim.x;
    const unsigned per = nblk / 8U, rem = nblk % 8U;
    const unsigned xcd = blockIdx.x % 8U, slot = blockIdx.x / 8U;
    // XCD x owns per + (x < rem) workgroups, laid out one range after the other
    return xcd * per + (xcd < rem ? xcd : rem) + slot;
}

#endif
}  // namespace rocco
