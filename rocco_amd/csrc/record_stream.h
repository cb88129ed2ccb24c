// rocco_amd/csrc/record_stream.h -- what count.hip, interval_count.hip and fragment_length.hip share around their
// concatenated records (T tracks, T + 1 offsets): the bisections, two wavefront reductions and the host's check of the
// offsets.  Header only.
#pragma once

#include "common.h"

namespace rocco {

namespace {

// largest t in [0, T) with offsets[t] <= item (offsets has T + 1 ascending entries, item < offsets[T]): entries without
// work are skipped
template <class Offset>
__device__ __forceinline__ int find_slot(const Offset *__restrict__ offsets, int T, Offset item)
{
    int lo = 0, hi = T;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= item) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// first index in [lo, hi) with pos[index] >= key (hi where none)
__device__ __forceinline__ long long lower_bound_pos(const int *__restrict__ pos, long long lo, long long hi, long long key)
{
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)pos[mid] < key) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// a thread's lowest index (~0: none) and highest index + 1 (0: none) over its wavefront, then into *first_out / *last_out
// with one atomic each
__device__ __forceinline__ void wave_first_last(unsigned long long first, unsigned long long last,
                                                unsigned long long *__restrict__ first_out, unsigned long long *__restrict__ last_out)
{
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const unsigned long long f = __shfl_xor(first, off), l = __shfl_xor(last, off);
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (first != ~0ULL) {
            atomicMin(first_out, first);
        }
        if (last != 0) {
            atomicMax(last_out, last);
        }
    }
}

// ... into result[0] / result[1]
__device__ __forceinline__ void wave_first_last(unsigned long long first, unsigned long long last,
                                                unsigned long long *__restrict__ result)
{
    wave_first_last(first, last, result, result + 1);
}

// T in [1, 2^31), offsets from 0 upwards, every track with fewer than 2^31 records
inline int check_record_tracks(const int64_t *rec_offsets_host, size_t T, const char *who)
{
    bool ok = T > 0 && T < (size_t)0x7fffffff && rec_offsets_host[0] >= 0;
    for (size_t t = 0; ok && t < T; ++t) {
        const long long n = rec_offsets_host[t + 1] - rec_offsets_host[t];
        ok = n >= 0 && n < (1LL << 31);
    }
    if (!ok) {
        set_last_error(std::string(who) + ": the number of tracks or a track's record range is invalid");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

}  // namespace

}  // namespace rocco
