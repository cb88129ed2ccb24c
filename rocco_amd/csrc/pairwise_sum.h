// rocco_amd/csrc/pairwise_sum.h -- NumPy's pairwise sum (numpy/_core/src/umath/loops_utils.h.src), term(i) the i-th addend,
// written ONCE for the kernels of dispersion.hip and for tests/tools/pairwise_order_check.cpp, which runs this very code on the
// host against np.sum for every length up to kPairwiseMax.
//
// Fewer than 8 terms one after the other; up to 128 with eight interleaved accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder appended; longer ranges split at n/2 rounded down to a multiple of 8,
// each half summed the same way.  The recursion is written out to kPairwiseDepth levels (no call, no stack: a kernel that uses
// it keeps a private segment of 0 bytes).
//
// The halves are UNEVEN (the rounding to a multiple of 8), so the depth a length needs is not log2(n / 128): a range that is
// still longer than 128 terms when the written-out levels are used up would be summed as one block, which NumPy splits
// again.  The first length with such a leaf is 969 at depth 3 and 1929 at depth 4, so depth 4 serves every n <= 1024;
// kPairwiseMax is the documented limit of the entry points, not a function of the depth, and the static_assert below holds the
// two together.  Plain C++ besides the __host__ __device__ marks.
#pragma once

#if defined(__HIPCC__)
#define ROCCO_PAIRWISE_HD __host__ __device__ __forceinline__
#else
#define ROCCO_PAIRWISE_HD inline
#endif

namespace rocco {

constexpr int kPairwiseBlock = 128;  // NumPy's PW_BLOCKSIZE: the longest range summed without a split
constexpr int kPairwiseDepth = 4;    // levels of splitting that are written out
constexpr int kPairwiseMax = 1024;   // the longest column the entry points take (_PAIRWISE_MAX_K of rocco_amd/rocco.py)

// the longest range left unsplit when n terms are split `depth` times at the most
constexpr int pairwise_longest_leaf(int n, int depth)
{
    if (depth == 0 || n <= kPairwiseBlock) {
        return n;
    }
    const int n2 = n / 2 - (n / 2) % 8;
    const int a = pairwise_longest_leaf(n2, depth - 1), b = pairwise_longest_leaf(n - n2, depth - 1);
    return a > b ? a : b;
}

constexpr bool pairwise_depth_serves(int longest, int depth)
{
    for (int n = 1; n <= longest; ++n) {
        if (pairwise_longest_leaf(n, depth) > kPairwiseBlock) {
            return false;
        }
    }
    return true;
}

static_assert(pairwise_depth_serves(kPairwiseMax, kPairwiseDepth),
              "a length up to kPairwiseMax leaves a block of more than 128 terms, which NumPy would split again");
static_assert(pairwise_depth_serves(968, 3) && !pairwise_depth_serves(969, 3) && pairwise_depth_serves(1928, 4) &&
                  !pairwise_depth_serves(1929, 4),
              "the bounds stated at the head of this file");

template <typename F>
ROCCO_PAIRWISE_HD double pairwise_block(int start, int n, F term)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) {
            res += term(start + i);
        }
        return res;
    }
    double r[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 8; ++q) {
        r[q] = term(start + q);
    }
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int q = 0; q < 8; ++q) {
            r[q] += term(start + i + q);
        }
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) {
        res += term(start + i);
    }
    return res;
}

template <int DEPTH, typename F>
ROCCO_PAIRWISE_HD double pairwise(int start, int n, F term)
{
    if constexpr (DEPTH == 0) {
        return pairwise_block(start, n, term);
    } else {
        if (n <= kPairwiseBlock) {
            return pairwise_block(start, n, term);
        }
        int n2 = n / 2;
        n2 -= n2 % 8;
        return pairwise<DEPTH - 1>(start, n2, term) + pairwise<DEPTH - 1>(start + n2, n - n2, term);
    }
}

}  // namespace rocco
