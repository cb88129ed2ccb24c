// rocco_amd/csrc/radix_key.h -- what the radix selects of wls.hip and select.hip share: the order-preserving key of a
// double and the contention-aware count into an LDS histogram.
#pragma once

#include "common.h"

namespace rocco {
#if defined(__HIPCC__)

// ascending keys <=> ascending doubles (-0.0 before +0.0); a NaN sorts by its sign bit like any other pattern
__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

__device__ __forceinline__ double key_to_double(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    return __longlong_as_double((long long)b);
}

// One count per active lane into an LDS histogram.  The keys of a row of counts, or the variances of one bin, crowd into a few
// buckets: 64 lanes adding to ONE counter are serialised lane by lane.  So the two most common buckets of the wavefront are
// counted by one lane each (a ballot of the lanes that share the leader's bucket), whoever is left adds for itself.
__device__ __forceinline__ void lds_count(unsigned *__restrict__ local, unsigned bucket, bool active)
{
    unsigned long long todo = __ballot(active);
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (todo == 0ULL) {
            break;
        }
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned b0 = (unsigned)__shfl((int)bucket, leader);
        const unsigned long long same = __ballot(active && bucket == b0) & todo;
        if (lane == leader) {
            atomicAdd(&local[b0], (unsigned)__popcll(same));
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ULL) {
        atomicAdd(&local[bucket], 1u);
    }
}

#endif
}  // namespace rocco
