// rocco_amd/csrc/select.hip -- order statistics of n-long score vectors without sorting them, and the elementwise passes
// behind them (gfx950).
//
// Replaces the n-long work of rocco/rocco.py:358-395 (cscores_quantiles: ten np.quantile(..., method="higher") per
// chromosome) and of rocco/inference.py:32-37, 382-443 (_robust_scale, benjamini_hochberg, _standardize_wls_z_scores,
// candidate_mask_from_wls): each is a few order statistics of a vector plus one elementwise pass.
//
// The select: a radix select over the order-preserving keys (radix_key.h) that follows up to 16 ranks of up to 48 vectors
// at once.  Six counting passes take 14, 10, 10, 10, 10 and 10 key bits from the top.  A pass reads every vector once
// (8 bytes per value; about 1024 workgroups dealt to the vectors by length, each taking chunks of 16384 values of its
// vector in turn) and counts, per vector, the digits of the keys that match one of the vector's still-distinct wanted
// prefixes ("slots": all ranks share one slot in pass 0, ranks that fall into one bucket keep sharing theirs) into an LDS
// histogram of 16384 counters -- one slot of 2^14 buckets in pass 0, up to sixteen of 2^10 afterwards -- and adds the
// non-zero ones to the vector's histogram in device memory.  A placement launch behind each pass (one workgroup per
// vector, one wavefront per rank) finds the bucket that holds each rank, appends its digit to the rank's prefix, renumbers
// the slots and clears the histogram; the last one turns the complete keys back into doubles.  13 launches per group of
// 48 vectors whatever the number of ranks, no host synchronisation, 16384 counters and one small state record per
// vector of scratch, nothing in proportion to n.  Every result follows from integer counts, so it does not depend on
// the order in which workgroups run.
//
// Every pass reads every value, whatever the data: 48 bytes per value in all, against the 128 and more a 64-bit radix
// sort moves.  A vector that is mostly one value (a score track of zeros) costs what any other costs -- its lanes meet in
// one bucket, which lds_count counts by ballot -- and there is no gather buffer to overflow.
#include "kernels.h"
#include "radix_key.h"

namespace rocco {

namespace {

constexpr int kChunk = ROCCO_SELECT_CHUNK_VALUES;     // values a workgroup of a counting pass takes at a time
constexpr int kGridTarget = ROCCO_SELECT_GRID_TARGET; // workgroups of a counting pass: two per CU at 64 KB of LDS each, twice over
constexpr int kCountThreads = ROCCO_SELECT_THREADS;   // threads of a counting workgroup (eight loads in flight each)
constexpr int kBhThreads = ROCCO_BH_THREADS, kBhMaxGrid = ROCCO_BH_MAX_GRID;
constexpr int kCounters = 16384;  // histogram counters per vector: 1 slot x 2^14 buckets, or up to 16 slots x 2^10
constexpr int kFirstBits = 14, kLaterBits = 10, kPasses = 6;
static_assert(kFirstBits + (kPasses - 1) * kLaterBits == 64, "the passes cover the key");
static_assert(kCountThreads == 256 && kChunk % (8 * kCountThreads) == 0 && kBhThreads == 256 && kGridTarget > 0 && kBhMaxGrid > 0,
              "rocco_hip.h states the shape");
static_assert((1 << kFirstBits) <= kCounters && kSelectRanksMax * (1 << kLaterBits) <= kCounters, "a vector's histogram");

constexpr unsigned long long kMagnitude = 0x7FFFFFFFFFFFFFFFULL, kInfBits = 0x7FF0000000000000ULL;
constexpr unsigned long long kNanKey = ~0ULL;  // every NaN: above +inf; key_to_double gives the quiet NaN 0x7FFF...F

struct SelectState {  // per vector, in device memory
    unsigned long long prefix[kSelectRanksMax];       // per rank: the bits of the wanted key found so far (right-aligned)
    unsigned long long slot_prefix[kSelectRanksMax];  // the distinct ones among them
    unsigned rank[kSelectRanksMax];                   // per rank: its rank among the keys that match its prefix
    int slot_of[kSelectRanksMax];
    int n_slots;
    int pad;
};

struct SelectBatch {  // kernel argument of the counting passes
    unsigned block_begin[kSelectBatchMax];  // first workgroup of every vector, ascending; unused entries 0xFFFFFFFF
    unsigned blocks[kSelectBatchMax];       // its workgroups: each takes every blocks-th chunk of the vector
    const double *x[kSelectBatchMax];
    double center[kSelectBatchMax];
    unsigned n[kSelectBatchMax];
    int n_vectors;
    int mode;
};

struct SelectRanks {  // kernel argument of the initialisation
    unsigned rank[kSelectBatchMax][kSelectRanksMax];
};

// mode 0: the key of x; mode 1: the key of |x - center|, a non-finite x keyed as a NaN
__device__ __forceinline__ unsigned long long select_key(double x, int mode, double center)
{
    unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    bool is_nan = (bits & kMagnitude) > kInfBits;
    if (mode == 1) {
        const bool non_finite = (bits & kMagnitude) >= kInfBits;
        const double d = fabs(x - center);
        bits = (unsigned long long)__double_as_longlong(d);
        is_nan = non_finite || (bits & kMagnitude) > kInfBits;
    }
    return is_nan ? kNanKey : order_key(__longlong_as_double((long long)bits));
}

__global__ __launch_bounds__(1024) void select_init_kernel(SelectRanks ranks, int n_ranks, SelectState *__restrict__ state,
                                                           unsigned *__restrict__ hist, long long *__restrict__ counts)
{
    const int v = blockIdx.x;
    const int t = threadIdx.x;
    if (t < kSelectRanksMax) {
        state[v].prefix[t] = 0ULL;
        state[v].slot_prefix[t] = 0ULL;
        state[v].rank[t] = (t < n_ranks) ? ranks.rank[v][t] : 0u;
        state[v].slot_of[t] = 0;
    }
    if (t == 0) {
        state[v].n_slots = 1;
    }
    if (t < 4) {
        counts[4 * v + t] = 0;
    }
    unsigned *__restrict__ mine = hist + (long long)v * kCounters;
    for (int b = t; b < kCounters; b += 1024) {
        mine[b] = 0u;
    }
}

// One pass: hist[vector][slot * 2^width + digit] += the keys of the vector that match the slot's prefix, digit = the `width`
// bits above bit `low`.  FIRST (pass 0: no prefix yet, one slot) also counts the NaNs, the infinities of either sign and the
// non-NaN values <= 0.0 of the vector itself.
template <bool FIRST>
__global__ __launch_bounds__(256) void select_count_kernel(SelectBatch batch, int low, int width, const SelectState *__restrict__ state,
                                                          unsigned *__restrict__ hist, long long *__restrict__ counts)
{
    __shared__ unsigned local[kCounters];
    int v = 0;
    for (int t = 1; t < batch.n_vectors; ++t) {
        v = (batch.block_begin[t] <= blockIdx.x) ? t : v;
    }
    const double *__restrict__ x = batch.x[v];
    const long long n = (long long)batch.n[v];
    const double center = batch.center[v];
    const int mode = batch.mode;
    const long long first = (long long)(blockIdx.x - batch.block_begin[v]) * kChunk;
    const long long stride = (long long)batch.blocks[v] * kChunk;
    const SelectState *__restrict__ st = state + v;
    const int n_slots = FIRST ? 1 : st->n_slots;
    const int used = n_slots << width;  // counters of this pass (at most kCounters)
    for (int b = threadIdx.x; b < used; b += 256) {
        local[b] = 0u;
    }
    __syncthreads();
    const int above_bits = low + width;  // the prefixes hold the bits above_bits .. 63
    const unsigned long long mask = (1ULL << width) - 1ULL;
    unsigned n_nan = 0u, n_ninf = 0u, n_pinf = 0u, n_le0 = 0u;
    // A workgroup counts several chunks into one LDS histogram before it adds to the vector's: the adds to device memory (one
    // per non-zero counter: thousands per workgroup while the wanted prefixes are short) and the clearing are paid once.
    // (eight loads in flight per thread, at clamped positions: a load under `if (i < n)` is waited for before the next is issued)
    for (long long base = first; base < n; base += stride)
    for (int j0 = 0; j0 < kChunk / 256; j0 += 8) {
        if (base + 256LL * j0 >= n) {
            break;
        }
        double val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = base + threadIdx.x + 256LL * (j0 + u);
            val[u] = x[(i < n) ? i : (n - 1)];
        }
        unsigned long long key[8];
        int slot[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            key[u] = select_key(val[u], mode, center);
            slot[u] = FIRST ? 0 : -1;
        }
        if (FIRST) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long long i = base + threadIdx.x + 256LL * (j0 + u);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(val[u]);
                const bool is_nan = (bits & kMagnitude) > kInfBits;
                const bool in = i < n;
                n_nan += (in && is_nan) ? 1u : 0u;
                n_ninf += (in && bits == (kInfBits | 0x8000000000000000ULL)) ? 1u : 0u;
                n_pinf += (in && bits == kInfBits) ? 1u : 0u;
                n_le0 += (in && !is_nan && ((bits >> 63) != 0ULL || (bits & kMagnitude) == 0ULL)) ? 1u : 0u;
            }
        } else {
            for (int s = 0; s < n_slots; ++s) {
                const unsigned long long wanted = st->slot_prefix[s];  // (uniform: a scalar load)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    slot[u] = ((key[u] >> above_bits) == wanted) ? s : slot[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = base + threadIdx.x + 256LL * (j0 + u);
            const bool counted = i < n && slot[u] >= 0;
            const unsigned bucket = ((unsigned)(counted ? slot[u] : 0) << width) | (unsigned)((key[u] >> low) & mask);
            lds_count(local, bucket, counted);
        }
    }
    __syncthreads();
    unsigned *__restrict__ mine = hist + (long long)v * kCounters;
    for (int b = threadIdx.x; b < used; b += 256) {
        const unsigned c = local[b];
        if (c != 0u) {
            atomicAdd(&mine[b], c);
        }
    }
    if (FIRST) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n_nan += __shfl_xor(n_nan, off);
            n_ninf += __shfl_xor(n_ninf, off);
            n_pinf += __shfl_xor(n_pinf, off);
            n_le0 += __shfl_xor(n_le0, off);
        }
        if ((threadIdx.x & 63) == 0) {
            unsigned long long *__restrict__ c = (unsigned long long *)(counts + 4 * v);
            if (n_nan != 0u) atomicAdd(&c[0], (unsigned long long)n_nan);
            if (n_ninf != 0u) atomicAdd(&c[1], (unsigned long long)n_ninf);
            if (n_pinf != 0u) atomicAdd(&c[2], (unsigned long long)n_pinf);
            if (n_le0 != 0u) atomicAdd(&c[3], (unsigned long long)n_le0);
        }
    }
}

// Behind a pass, one workgroup per vector and one wavefront per rank: the digit of the bucket that holds the rank joins
// the rank's prefix, the rank becomes the rank inside that bucket; then the distinct prefixes are numbered as the slots of
// the next pass and the histogram is cleared.  LAST: the prefixes are whole keys, written out as doubles.
__global__ __launch_bounds__(1024) void select_place_kernel(SelectState *__restrict__ state, unsigned *__restrict__ hist, int width,
                                                            int n_ranks, int last, double *__restrict__ values_out)
{
    __shared__ unsigned long long new_prefix[kSelectRanksMax];
    __shared__ unsigned new_rank[kSelectRanksMax];
    const int v = blockIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    SelectState *__restrict__ st = state + v;
    unsigned *__restrict__ mine = hist + (long long)v * kCounters;
    if (w < n_ranks) {
        const int per = (1 << width) / 64;  // consecutive buckets per lane
        const unsigned rank = st->rank[w];
        const unsigned *__restrict__ h = mine + ((long long)st->slot_of[w] << width) + lane * per;
        unsigned sum = 0u;
        for (int q = 0; q < per; ++q) {
            sum += h[q];
        }
        unsigned incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned other = __shfl_up(incl, off);
            incl += (lane >= off) ? other : 0u;
        }
        const unsigned excl = incl - sum;
        // exactly one lane: the slot's buckets hold more keys than the rank (the last lane takes what a miscount would leave over)
        if (rank >= excl && (rank < incl || lane == 63)) {
            unsigned r = rank - excl;
            int q = 0;
            while (q < per - 1 && h[q] <= r) {
                r -= h[q];
                ++q;
            }
            new_prefix[w] = (st->prefix[w] << width) | (unsigned long long)(lane * per + q);
            new_rank[w] = r;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n_slots = 0;
        for (int r = 0; r < n_ranks; ++r) {
            const unsigned long long p = new_prefix[r];
            int s = 0;
            while (s < n_slots && st->slot_prefix[s] != p) {
                ++s;
            }
            if (s == n_slots) {
                st->slot_prefix[n_slots++] = p;
            }
            st->prefix[r] = p;
            st->rank[r] = new_rank[r];
            st->slot_of[r] = s;
            if (last) {
                values_out[(long long)v * n_ranks + r] = key_to_double(p);
            }
        }
        st->n_slots = n_slots;
    }
    if (!last) {
        for (int b = threadIdx.x; b < kCounters; b += 1024) {
            mine[b] = 0u;
        }
    }
}

// The last element of the sorted copy that passes sorted[i] <= fdr * ((k + 1) / m) (inference.py:394-398), as its index i;
// *index_out starts at -1.  k is the element's rank in the REFERENCE's order, where np.argsort puts every NaN last:
// rocco_hip_sort_f64 sorts bit patterns, so the NaNs whose sign bit is set (what 0.0 / 0.0 gives on x86-64) lead the sorted
// copy, `lead` of them, and k = i - lead.  They form a prefix: every thread finds its end by the same bisection (uniform
// addresses: one cache line per step).  No NaN of either sign passes a comparison.
__global__ __launch_bounds__(256) void bh_last_passing_kernel(const double *__restrict__ sorted, long long m, double fdr,
                                                             long long *__restrict__ index_out)
{
    long long lead = 0, end = m;  // sorted[i] is a sign-set NaN for i < lead, is none for i >= end
    while (lead < end) {
        const long long mid = lead + (end - lead) / 2;
        const bool leading_nan = (unsigned long long)__double_as_longlong(sorted[mid]) > (kInfBits | 0x8000000000000000ULL);
        lead = leading_nan ? mid + 1 : lead;
        end = leading_nan ? end : mid;
    }
    long long best = -1;
    const double md = (double)m;
    for (long long i = lead + (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
        const double threshold = fdr * ((double)(i - lead + 1) / md);
        best = (sorted[i] <= threshold) ? i : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long other = __shfl_xor(best, off);
        best = (other > best) ? other : best;
    }
    if ((threadIdx.x & 63) == 0 && best >= 0) {
        atomicMax(index_out, best);
    }
}

__device__ __forceinline__ bool is_finite_bits(double x)
{
    return ((unsigned long long)__double_as_longlong(x) & kInfBits) != kInfBits;
}

__global__ __launch_bounds__(256) void threshold_mask_kernel(const double *__restrict__ x, long long n, double divisor, double threshold,
                                                            double floor_value, int use_floor, uint8_t *__restrict__ mask)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const double v = x[i];
    const double standardized = is_finite_bits(v) ? v / divisor : 0.0;
    mask[i] = (uint8_t)((standardized > threshold && (use_floor == 0 || v > floor_value)) ? 1 : 0);
}

__global__ __launch_bounds__(256) void at_most_mask_kernel(const double *__restrict__ x, long long n, double cutoff,
                                                          uint8_t *__restrict__ mask)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        mask[i] = (uint8_t)((x[i] <= cutoff) ? 1 : 0);
    }
}

__global__ __launch_bounds__(256) void divide_finite_kernel(const double *__restrict__ x, long long n, double divisor,
                                                           double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double v = x[i];
        out[i] = is_finite_bits(v) ? v / divisor : 0.0;
    }
}

constexpr size_t kStateBytes = ((sizeof(SelectState) * kSelectBatchMax + 255) / 256) * 256;

}  // namespace

size_t select_scratch_bytes(size_t count)
{
    const size_t group = count < (size_t)kSelectBatchMax ? count : (size_t)kSelectBatchMax;
    return kStateBytes + group * kCounters * sizeof(unsigned);
}

int launch_select_ranks_batch(const double *const *vectors_dev, const size_t *n, size_t count, int n_ranks, const long long *ranks,
                              int mode, const double *centers, double *values_out_dev, long long *counts_out_dev, void *scratch_dev,
                              hipStream_t stream)
{
    SelectState *state = (SelectState *)scratch_dev;
    unsigned *hist = (unsigned *)((char *)scratch_dev + kStateBytes);
    // (the groups use the same scratch one after the other: they are queued on one stream)
    for (size_t v0 = 0; v0 < count; v0 += kSelectBatchMax) {
        const int g = (int)((count - v0 < (size_t)kSelectBatchMax) ? count - v0 : (size_t)kSelectBatchMax);
        SelectBatch batch;
        SelectRanks first;
        std::memset(&first, 0, sizeof(first));
        unsigned blocks = 0;
        size_t group_total = 0;
        for (int t = 0; t < g; ++t) {
            group_total += n[v0 + t];
        }
        for (int t = 0; t < kSelectBatchMax; ++t) {
            const bool live = t < g;
            batch.block_begin[t] = live ? blocks : 0xFFFFFFFFu;
            batch.x[t] = live ? vectors_dev[v0 + t] : nullptr;
            batch.center[t] = (live && mode == 1) ? centers[v0 + t] : 0.0;
            batch.n[t] = live ? (unsigned)n[v0 + t] : 0u;
            batch.blocks[t] = 0u;
            if (live) {
                // about kGridTarget workgroups in all, dealt by length; never more than the vector has chunks
                const size_t chunks = (n[v0 + t] + kChunk - 1) / kChunk;
                const size_t share = (size_t)((double)kGridTarget * (double)n[v0 + t] / (double)(group_total > 0 ? group_total : 1)) + 1;
                batch.blocks[t] = (unsigned)(chunks < share ? chunks : share);
                blocks += batch.blocks[t];
                for (int r = 0; r < n_ranks; ++r) {
                    first.rank[t][r] = (unsigned)ranks[(v0 + t) * n_ranks + r];
                }
            }
        }
        batch.n_vectors = g;
        batch.mode = mode;
        long long *counts = counts_out_dev + 4 * v0;
        double *values = (n_ranks > 0) ? values_out_dev + v0 * n_ranks : nullptr;
        hipLaunchKernelGGL(select_init_kernel, dim3(g), dim3(1024), 0, stream, first, n_ranks, state, hist, counts);
        if (blocks == 0) {
            continue;
        }
        const int passes = (n_ranks > 0) ? kPasses : 1;  // (no rank wanted: pass 0 for the counts alone)
        int low = 64;
        for (int p = 0; p < passes; ++p) {
            const int width = (p == 0) ? kFirstBits : kLaterBits;
            low -= width;
            if (p == 0) {
                hipLaunchKernelGGL(select_count_kernel<true>, dim3(blocks), dim3(256), 0, stream, batch, low, width, state, hist, counts);
            } else {
                hipLaunchKernelGGL(select_count_kernel<false>, dim3(blocks), dim3(256), 0, stream, batch, low, width, state, hist, counts);
            }
            if (n_ranks > 0) {
                hipLaunchKernelGGL(select_place_kernel, dim3(g), dim3(1024), 0, stream, state, hist, width, n_ranks,
                                   (p == passes - 1) ? 1 : 0, values);
            }
        }
    }
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

int launch_bh_last_passing_rank(const double *sorted_dev, size_t m, double fdr, long long *rank_out_dev, hipStream_t stream)
{
    ROCCO_HIP_TRY(hipMemsetAsync(rank_out_dev, 0xFF, sizeof(long long), stream));  // -1
    if (m == 0) {
        return ROCCO_HIP_OK;
    }
    const size_t want = (m + 255) / 256;
    const unsigned grid = (unsigned)(want < (size_t)kBhMaxGrid ? want : (size_t)kBhMaxGrid);
    hipLaunchKernelGGL(bh_last_passing_kernel, dim3(grid), dim3(256), 0, stream, sorted_dev, (long long)m, fdr, rank_out_dev);
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

int launch_threshold_mask(const double *x_dev, size_t n, double divisor, double threshold, double floor_value, int use_floor,
                          uint8_t *mask_out_dev, hipStream_t stream)
{
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    hipLaunchKernelGGL(threshold_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x_dev, (long long)n, divisor,
                       threshold, floor_value, use_floor, mask_out_dev);
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

int launch_at_most_mask(const double *x_dev, size_t n, double cutoff, uint8_t *mask_out_dev, hipStream_t stream)
{
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    hipLaunchKernelGGL(at_most_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x_dev, (long long)n, cutoff,
                       mask_out_dev);
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

int launch_divide_finite(const double *x_dev, size_t n, double divisor, double *out_dev, hipStream_t stream)
{
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    hipLaunchKernelGGL(divide_finite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x_dev, (long long)n, divisor,
                       out_dev);
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

}  // namespace rocco
