// rocco_amd/csrc/dispersion.hip -- column-wise dispersion over K samples (K x n row-major -> n), gfx950.
//
// Replaces rocco/rocco.py:307-355 (score_dispersion_chrom): stats.median_abs_deviation, stats.iqr, np.std and the
// per-column stats.tstd, each over axis 0 and each bit for bit as NumPy 2.2 / SciPy 1.15 compute it.
//
// 2 <= K <= 100: one launch that reads the matrix once, one lane per locus, the column in registers -- the layout of
// median.hip (row k is a coalesced segment per wavefront, workgroups in XCD-contiguous order, K padded to a network
// size).  Algorithmic bytes per locus (f64; f32 halves the reads):
//   mad   8 K read + 8 written   median network, |v - median| in place, median network again
//   iqr   8 K read + 8 written   complete sort, four order statistics picked by index
//   std   8 K read + 8 written   two passes over the registers in row order, no network
//   tstd  8 K read + 8 written   complete sort for the two limits; the masked sums then walk the column in ROW order,
//                                which the sort has destroyed.  Where the registers allow, an unpermuted copy is kept
//                                beside the network (2 x 200 VGPRs at K = 100: the copy sits in the accumulation
//                                registers, one wavefront per SIMD as median_kernel at K = 100 has anyway).  Only for
//                                80 < K < 100 (padded loads, whose bookkeeping no longer fits beside two copies) the
//                                column is READ A SECOND TIME into the sorted registers instead: 16 K read, of which
//                                the second 8 K follow the first from the same workgroup (a cache hit where the
//                                256 x K tile is still resident).
// K > 100: rank counting and plain loops over memory (O(K^2) reads served from L1 / L2).  mad, iqr and the row-after-row
// std take any K; tstd and the std of a single column, which sum in NumPy's pairwise order, take K <= kPairwiseMax = 1024.
// NO speed claim is attached to that path.
//
// Every kernel here keeps its arrays in registers with compile-time indices and calls nothing recursive: the private
// segment is 0 bytes (NumPy's pairwise order is written out to kPairwiseDepth = 4 levels instead, see pairwise_sum.h:
// NumPy's halves are uneven, and three levels leave a block of more than 128 terms from K = 969 on).
#include "kernels.h"
#include "pairwise_sum.h"
#include "select_network.h"

#include <limits>

namespace rocco {

namespace {

constexpr int kMad = 0, kIqr = 1, kStd = 2, kTstd = 3;
constexpr int kNetworkMax = 100;  // largest column the register kernels take

// The answer for a column that holds a NaN.  Written out where it is used, never returned from a function of this file:
// under -fno-honor-nans a function's double result is declared NaN-free, and a result known to be NaN is folded away.
#define ROCCO_QUIET_NAN __longlong_as_double(0x7FF8000000000000LL)

// A COMPUTED value whose bit pattern is to be tested goes through an empty asm statement first: this file's arithmetic is
// declared NaN-free, and what the compiler can trace of a result's origin it may use on the bit tests.  Behind the asm
// statement they are the integer compares they are written as.  Statements, not functions: see ROCCO_QUIET_NAN.
#define ROCCO_OPAQUE(variable) asm volatile("" : "+v"(variable))
#define ROCCO_COMPUTED_IS_NAN(flag, value)                                                                                     \
    do {                                                                                                                       \
        double probe_ = (value);                                                                                               \
        ROCCO_OPAQUE(probe_);                                                                                                  \
        (flag) = is_nan_bits(probe_);                                                                                          \
    } while (0)

// the upper 32 bits of |x|: at least kNonFiniteTop exactly for an infinity or a NaN
constexpr unsigned kNonFiniteTop = 0x7FF00000U;
__device__ __forceinline__ unsigned magnitude_top(double x)
{
    return (unsigned)((unsigned long long)__double_as_longlong(x) >> 32) & 0x7FFFFFFFU;
}

// FOR VALUES THAT ARE NO NaN ONLY (the limits of tstd: entries of a column without NaN).  The compiler recognises every
// test of the exponent bits, and the hardware class test too, as a class test and -- the file being declared NaN-free --
// compiles it to the floating-point compare |x| != inf, which calls a NaN finite; an empty asm statement on the way does
// not help.  What survives as written are is_nan_bits() (an integer compare) and is_inf_bits(): a value that may be NaN is
// asked those two, one after the other (the median of MAD, which is NaN for -inf and +inf in the middle).
__device__ __forceinline__ bool is_finite_bits(double x)
{
    return (__double_as_longlong(x) & 0x7FF0000000000000LL) != 0x7FF0000000000000LL;
}

// +inf or -inf; false for a NaN, also where it is compiled to |x| == inf
__device__ __forceinline__ bool is_inf_bits(double x)
{
    return (__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFLL) == 0x7FF0000000000000LL;
}

// tstd: the answer where the arithmetic does not give it.  The limits are the smallest and the largest kept value, so an
// infinite limit is a kept infinity and the mean is infinite with it.  SciPy 1.15 (stats.tvar -> _xp_var with
// nan_policy="omit") leaves the NaN deviations (inf - inf) OUT of the second mean: with one infinite limit the finite
// kept values are infinitely far from the mean and the variance is +inf; with two (of either signs) no deviation is
// left, or the mean itself is NaN: NaN.  Finite kept values CAN give NaN as well, in NumPy as here: the pairwise order
// keeps eight accumulators, and on entries near the overflow threshold of alternating sign (+-1.5e308, K >= 16) one of
// them reaches +inf and its neighbour -inf.  That NaN is not decided here: it comes out of the additions of `computed`
// themselves, which the hardware performs as IEEE 754 states whatever the compiler may assume.  The same overflow beside
// ONE infinite limit (a kept -inf, finite kept values whose sum reaches +inf) makes the mean NaN, every deviation with it,
// and SciPy's answer NaN instead of +inf: `mean_is_nan`, from ROCCO_COMPUTED_IS_NAN.  Everything else is decided on the
// bit patterns of the limits, never by testing `computed`.  Stores to `r` instead of returning, see ROCCO_QUIET_NAN.
#define trimmed_result(column_has_nan, mean_is_nan, kept_count, lo, hi, computed)                                            \
    (((column_has_nan) || (mean_is_nan) || (kept_count) <= 1.0 || (!is_finite_bits(lo) && !is_finite_bits(hi)))               \
         ? ROCCO_QUIET_NAN                                                                                                    \
         : ((!is_finite_bits(lo) || !is_finite_bits(hi)) ? std::numeric_limits<double>::infinity() : (computed)))

// np.percentile's linear rule between the sorted neighbours a <= b at fraction g (numpy/lib/_function_base_impl.py
// _lerp): a + (b - a) g below one half, b - (b - a) (1 - g) from one half on
__device__ __forceinline__ double lerp(double a, double b, double g)
{
    const double d = b - a;
    return (g >= 0.5) ? (b - d * (1.0 - g)) : (a + d * g);
}

// NumPy's pairwise sum over memory -- pairwise_block(), pairwise<DEPTH>() and kPairwiseDepth / kPairwiseMax -- is in
// pairwise_sum.h, which a host program compiles too (tests/tools/pairwise_order_check.cpp).

// the same order over the first K (<= KP <= 128) entries of a register array: every index a compile-time constant, the
// conditions on K uniform across the wavefront
template <int KP, typename F>
__device__ __forceinline__ double pairwise_registers(const double (&v)[KP], int K, F f)
{
    static_assert(KP <= 128, "one block of NumPy's pairwise sum");
    double res = 0.0;
    if (K < 8) {
#pragma unroll
        for (int i = 0; i < (KP < 7 ? KP : 7); ++i) {
            if (i < K) {
                res += f(v[i]);
            }
        }
        return res;
    }
    if constexpr (KP >= 8) {
        const int full = K - (K % 8);
        double r[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            r[q] = f(v[q]);
        }
#pragma unroll
        for (int i = 8; i + 8 <= KP; i += 8) {
            if (i < full) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    r[q] += f(v[i + q]);
                }
            }
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = 8; i < KP; ++i) {
            if (i >= full && i < K) {
                res += f(v[i]);
            }
        }
    }
    return res;
}

// ---- 2 <= K <= 100: the column in registers ----------------------------------------------------------------------

// rows 0..K-1 of column col0 + lane into v[0..K).  EXACT: K == KP is known at compile time (unpredicated loads).  Every
// row is read at (scalar row base) + (one 32-bit vector offset) and every load is unconditional (a load under a per-row
// condition is waited for before the next is issued): slots past the matrix re-read its last row (a cache hit) and are
// replaced by the caller.
template <typename T, int KP, bool EXACT>
__device__ __forceinline__ void load_column(const T *__restrict__ m, int K, long long stride, long long col0, unsigned lane,
                                            double (&v)[KP])
{
    const T *row = m + col0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        v[k] = (double)row[lane];
        row += (EXACT || k + 1 < K) ? stride : 0;
    }
}

// v[k >= K] = the padding, NaNs parked at +inf (the network must not see one); returns whether the column held a NaN.
// n_lo: how many padding entries are -inf (the others are +inf).
template <int KP, bool EXACT>
__device__ __forceinline__ bool pad_and_park(double (&v)[KP], int K, int n_lo)
{
    const double inf = std::numeric_limits<double>::infinity();
    double sum = 0.0;  // NaN in the column <=> NaN sum (or +inf and -inf together: checked below)
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (EXACT || k < K) {
            sum += v[k];
        } else {
            v[k] = (k - K < n_lo) ? -inf : inf;
        }
    }
    bool has_nan = false;
    if (is_nan_bits(sum)) {  // rare
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (EXACT || k < K) {
                const bool bad = is_nan_bits(v[k]);
                has_nan |= bad;
                v[k] = bad ? inf : v[k];
            }
        }
    }
    return has_nan;
}

// v[idx] for an index known only at run time, with every register index a compile-time constant: the bit patterns
// are masked and OR-ed together.  (A chain of selects `r = (k == idx) ? v[k] : r` is folded back into v[idx] by the
// compiler, and a dynamically indexed array lives in scratch memory.)
template <int KP>
__device__ __forceinline__ double pick(const double (&v)[KP], int idx)
{
    long long bits = 0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        bits |= __double_as_longlong(v[k]) & -(long long)(k == idx);
    }
    return __longlong_as_double(bits);
}

// tstd: whether the sums read the column again instead of keeping an unpermuted copy in registers
template <int KP, bool EXACT>
constexpr bool kRereadForSums = (KP > 80 && !EXACT);

struct DispersionArgs {
    int index0, index1;  // iqr: position of the lower neighbour of each percentile in the sorted column; tstd: the two ranks
    double g0, g1;       // iqr: the fraction between the neighbours; tstd: g0 != 0 takes the root of the variance
};

template <typename T, int KP, bool EXACT, int METHOD>
__global__ __launch_bounds__(256) void dispersion_kernel(const T *__restrict__ m, int K_runtime, long long n, long long stride,
                                                         DispersionArgs args, double *__restrict__ out)
{
    const long long col0 = (long long)xcd_contiguous_block() * 256;
    const unsigned lane = threadIdx.x;
    const long long j = col0 + lane;
    if (j >= n) {
        return;
    }
    const int K = EXACT ? KP : K_runtime;
    [[maybe_unused]] const double inf = std::numeric_limits<double>::infinity();
    double v[KP];
    load_column<T, KP, EXACT>(m, K, stride, col0, lane, v);
    double r;
    if constexpr (METHOD == kStd) {
        // np.std(m, axis=0): the rows added one after the other, one division; the squared deviations the same way
        double acc = v[0];
        unsigned top = magnitude_top(v[0]);
#pragma unroll
        for (int k = 1; k < KP; ++k) {
            if (EXACT || k < K) {
                acc += v[k];
                top = max(top, magnitude_top(v[k]));
            }
        }
        const double mean = acc / (double)K;
        const double d0 = v[0] - mean;
        acc = d0 * d0;
#pragma unroll
        for (int k = 1; k < KP; ++k) {
            if (EXACT || k < K) {
                const double d = v[k] - mean;
                acc += d * d;
            }
        }
        // In this order (one accumulator, row after row) NumPy answers NaN exactly when the column holds a NaN or an
        // infinity (inf - inf among the deviations): finite entries give no NaN here, an overflowing sum stays +inf.  (Not
        // so in the pairwise order of std_loop_kernel and of tstd, see trimmed_result.)  Decided on the entries' bit
        // patterns, not on the sum: this file's arithmetic is declared NaN-free, so no result of it is tested for being one.
        r = (top >= kNonFiniteTop) ? ROCCO_QUIET_NAN : sqrt(acc / (double)K);
    } else if constexpr (METHOD == kMad) {
        // K is padded to the even network size with -inf / +inf in equal numbers (one extra +inf for odd K), which
        // leaves the middle order statistics where they are
        const int n_lo = (KP - K) / 2;
        const bool has_nan = pad_and_park<KP, EXACT>(v, K, n_lo);
        select_middle<KP>(v);
        double med = (K & 1) ? v[KP / 2 - 1] : (v[KP / 2 - 1] + v[KP / 2]) / 2.0;
        // (-inf + +inf) / 2 is NaN: the bit tests below must see the register, not a result "that is never NaN"
        ROCCO_OPAQUE(med);
        const bool med_is_nan = is_nan_bits(med), med_is_inf = is_inf_bits(med);  // asked separately, see is_finite_bits
        // A median that is not finite (rare).  NaN: +inf and -inf in the middle.  Infinite: where an ENTRY is that same
        // infinity its deviation is inf - inf and np.median answers NaN; where none is -- the two middle values are finite and
        // their sum overflowed -- every deviation is +inf and so is the answer.  The entries are counted on their bit patterns,
        // less the padding of that sign.
        bool undefined = has_nan || med_is_nan;
        if (med_is_inf) {
            const long long med_bits = __double_as_longlong(med);
            int equal = 0;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                equal += (__double_as_longlong(v[k]) == med_bits) ? 1 : 0;
            }
            const int padded = EXACT ? 0 : ((med_bits < 0) ? n_lo : KP - K - n_lo);
            undefined = undefined || equal > padded;
        }
        // The network has permuted the registers but kept the multiset, which is all the second median needs.  The
        // padding must stay balanced: |+inf - med| is +inf again, and of the entries that come out as -inf (padding and
        // data alike: equal values) the first n_lo stay -inf while the others, data, become +inf.
        int seen = 0;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const double d = v[k] - med;
            if (EXACT) {
                v[k] = fabs(d);
            } else {
                const bool low = (d == -inf);
                v[k] = (low && seen < n_lo) ? d : fabs(d);
                seen += low ? 1 : 0;
            }
        }
        select_middle<KP>(v);
        r = (K & 1) ? v[KP / 2 - 1] : (v[KP / 2 - 1] + v[KP / 2]) / 2.0;
        // (around a median that is not finite the registers above held inf - inf: answered from the count, not from them)
        r = undefined ? ROCCO_QUIET_NAN : (med_is_inf ? inf : r);
    } else {
        // all of the padding is +inf: position i of the sorted registers is position i of the sorted column
        [[maybe_unused]] double rows[(METHOD == kTstd && !kRereadForSums<KP, EXACT>) ? KP : 1];  // tstd: the column in row order
        if constexpr (METHOD == kTstd && !kRereadForSums<KP, EXACT>) {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                rows[k] = v[k];
            }
        }
        const bool has_nan = pad_and_park<KP, EXACT>(v, K, 0);
        select_middle<KP>(v);  // every output can be picked below: a complete sort
        if constexpr (METHOD == kIqr) {
            const double a0 = pick<KP>(v, args.index0), b0 = pick<KP>(v, min(args.index0 + 1, K - 1));
            const double a1 = pick<KP>(v, args.index1), b1 = pick<KP>(v, min(args.index1 + 1, K - 1));
            r = lerp(a1, b1, args.g1) - lerp(a0, b0, args.g0);
            r = has_nan ? ROCCO_QUIET_NAN : r;
        } else {
            // stats.tstd(column, limits=(lo, hi), inclusive=(True, True)) of SciPy 1.15: values outside the limits count
            // as 0.0 in both sums, each summed in NumPy's pairwise order over the K entries in ROW order
            const double lo = pick<KP>(v, args.index0), hi = pick<KP>(v, args.index1);
            if constexpr (kRereadForSums<KP, EXACT>) {
                // the second read (see the head of this file).  The pointer is passed through an empty asm statement:
                // otherwise the compiler recognises the addresses of the first read and keeps those values alive
                const T *again = m;
                asm volatile("" : "+s"(again));
                load_column<T, KP, EXACT>(again, K, stride, col0, lane, v);
            } else {
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    v[k] = rows[k];
                }
            }
            auto kept = [&](double x) -> bool { return !(x < lo || x > hi); };
            double cnt = 0.0;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (EXACT || k < K) {
                    cnt += kept(v[k]) ? 1.0 : 0.0;
                }
            }
            const double mean = pairwise_registers<KP>(v, K, [&](double x) { return kept(x) ? x : 0.0; }) / cnt;
            double var = pairwise_registers<KP>(v, K, [&](double x) {
                             const double d = x - mean;
                             return kept(x) ? d * d : 0.0;
                         }) / cnt;
            var *= cnt / (cnt - 1.0);
            bool mean_is_nan;
            ROCCO_COMPUTED_IS_NAN(mean_is_nan, mean);
            r = trimmed_result(has_nan, mean_is_nan, cnt, lo, hi, args.g0 != 0.0 ? sqrt(var) : var);
        }
    }
    out[j] = r;
}

// ---- any K: rank counting and plain loops over memory (no speed claim) --------------------------------------------

// the values at the sorted positions want[0..W) of the column; false if the column holds a NaN.  `value(k)` is entry k.
template <int W, typename F>
__device__ __forceinline__ bool order_statistics(int K, const int (&want)[W], double (&found)[W], F value)
{
    bool has_nan = false;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        found[w] = 0.0;
    }
    for (int a = 0; a < K; ++a) {
        const double x = value(a);
        if (is_nan_bits(x)) {
            has_nan = true;
            continue;
        }
        int less = 0, equal = 0;
        for (int b = 0; b < K; ++b) {
            const double y = value(b);
            less += (y < x);
            equal += (y == x);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (want[w] >= less && want[w] < less + equal) {  // x occupies the sorted positions [less, less + equal)
                found[w] = x;
            }
        }
    }
    return !has_nan;
}

template <typename T, int METHOD>
__global__ __launch_bounds__(256) void dispersion_rank_kernel(const T *__restrict__ m, int K, long long n, long long stride,
                                                              DispersionArgs args, double *__restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) {
        return;
    }
    const T *__restrict__ col = m + j;
    auto entry = [&](int k) -> double { return (double)col[(long long)k * stride]; };
    double r;
    if constexpr (METHOD == kMad) {
        const int want[2] = {(K - 1) / 2, K / 2};
        double mid[2];
        bool ok = order_statistics<2>(K, want, mid, entry);
        double med = (K & 1) ? mid[0] : (mid[0] + mid[1]) / 2.0;
        ROCCO_OPAQUE(med);  // (as in dispersion_kernel)
        const bool med_is_nan = is_nan_bits(med), med_is_inf = is_inf_bits(med);  // asked separately, see is_finite_bits
        if (ok && !med_is_nan && !med_is_inf) {
            order_statistics<2>(K, want, mid, [&](int k) -> double { return fabs(entry(k) - med); });
            r = (K & 1) ? mid[0] : (mid[0] + mid[1]) / 2.0;
        } else {
            // a median that is not finite, as in dispersion_kernel: NaN where it is NaN or an entry is that same infinity,
            // +inf where the sum of two finite middle values overflowed
            bool undefined = !ok || med_is_nan;
            for (int k = 0; k < K; ++k) {
                undefined = undefined || (__double_as_longlong(entry(k)) == __double_as_longlong(med));
            }
            r = undefined ? ROCCO_QUIET_NAN : std::numeric_limits<double>::infinity();
        }
    } else if constexpr (METHOD == kIqr) {
        const int want[4] = {args.index0, min(args.index0 + 1, K - 1), args.index1, min(args.index1 + 1, K - 1)};
        double s[4];
        const bool ok = order_statistics<4>(K, want, s, entry);
        r = ok ? (lerp(s[2], s[3], args.g1) - lerp(s[0], s[1], args.g0)) : ROCCO_QUIET_NAN;
    } else {
        const int want[2] = {args.index0, args.index1};
        double lim[2];
        const bool ok = order_statistics<2>(K, want, lim, entry);
        const double lo = lim[0], hi = lim[1];
        auto kept = [&](double x) -> bool { return !(x < lo || x > hi); };
        double cnt = 0.0;
        for (int k = 0; k < K; ++k) {
            cnt += kept(entry(k)) ? 1.0 : 0.0;
        }
        const double mean = pairwise<kPairwiseDepth>(0, K, [&](int k) -> double {
                                const double x = entry(k);
                                return kept(x) ? x : 0.0;
                            }) / cnt;
        double var = pairwise<kPairwiseDepth>(0, K, [&](int k) -> double {
                         const double x = entry(k);
                         const double d = x - mean;
                         return kept(x) ? d * d : 0.0;
                     }) / cnt;
        var *= cnt / (cnt - 1.0);
        bool mean_is_nan;
        ROCCO_COMPUTED_IS_NAN(mean_is_nan, mean);
        r = trimmed_result(!ok, mean_is_nan, cnt, lo, hi, args.g0 != 0.0 ? sqrt(var) : var);
    }
    out[j] = r;
}

// np.std over memory.  PAIRWISE: both sums in NumPy's pairwise order (how NumPy reduces the single column of a K x 1
// matrix); otherwise the rows one after the other (how it reduces axis 0 of every wider matrix).
template <typename T, bool PAIRWISE>
__global__ __launch_bounds__(256) void std_loop_kernel(const T *__restrict__ m, int K, long long n, long long stride,
                                                       double *__restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) {
        return;
    }
    const T *__restrict__ col = m + j;
    auto entry = [&](int k) -> double { return (double)col[(long long)k * stride]; };
    double mean, acc;
    unsigned top = 0;
    for (int k = 0; k < K; ++k) {
        top = max(top, magnitude_top(entry(k)));
    }
    if constexpr (PAIRWISE) {
        mean = pairwise<kPairwiseDepth>(0, K, entry) / (double)K;
        acc = pairwise<kPairwiseDepth>(0, K, [&](int k) -> double {
            const double d = entry(k) - mean;
            return d * d;
        });
    } else {
        acc = entry(0);
        for (int k = 1; k < K; ++k) {
            acc += entry(k);
        }
        mean = acc / (double)K;
        const double d0 = entry(0) - mean;
        acc = d0 * d0;
        for (int k = 1; k < K; ++k) {
            const double d = entry(k) - mean;
            acc += d * d;
        }
    }
    out[j] = (top >= kNonFiniteTop) ? ROCCO_QUIET_NAN : sqrt(acc / (double)K);  // (as in dispersion_kernel)
}

template <typename T, int KP, int METHOD>
void launch_kp(const T *m, int K, long long n, long long stride, const DispersionArgs &args, double *out, hipStream_t stream)
{
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (K == KP) {
        hipLaunchKernelGGL((dispersion_kernel<T, KP, true, METHOD>), grid, block, 0, stream, m, K, n, stride, args, out);
    } else {
        hipLaunchKernelGGL((dispersion_kernel<T, KP, false, METHOD>), grid, block, 0, stream, m, K, n, stride, args, out);
    }
}

template <typename T, int METHOD>
int dispatch(const T *m, int K, long long n, long long stride, const DispersionArgs &args, double *out, hipStream_t stream)
{
    if (K <= 2) launch_kp<T, 2, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 4) launch_kp<T, 4, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 8) launch_kp<T, 8, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 12) launch_kp<T, 12, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 16) launch_kp<T, 16, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 24) launch_kp<T, 24, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 32) launch_kp<T, 32, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 48) launch_kp<T, 48, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 64) launch_kp<T, 64, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= 80) launch_kp<T, 80, METHOD>(m, K, n, stride, args, out, stream);
    else if (K <= kNetworkMax) launch_kp<T, kNetworkMax, METHOD>(m, K, n, stride, args, out, stream);
    else if constexpr (METHOD == kStd) {
        hipLaunchKernelGGL((std_loop_kernel<T, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, K, n, stride, out);
    } else {
        if (METHOD == kTstd && K > kPairwiseMax) {
            return ROCCO_HIP_EINVAL;
        }
        hipLaunchKernelGGL((dispersion_rank_kernel<T, METHOD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, K, n,
                           stride, args, out);
    }
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

template <int METHOD>
int launch(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, const DispersionArgs &args,
           double *scores_dev, hipStream_t stream)
{
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    if (dtype == 0) {
        return dispatch<double, METHOD>((const double *)matrix_dev, (int)K, (long long)n, (long long)row_stride, args, scores_dev,
                                        stream);
    }
    return dispatch<float, METHOD>((const float *)matrix_dev, (int)K, (long long)n, (long long)row_stride, args, scores_dev, stream);
}

}  // namespace

int launch_mad(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, double *scores_dev, hipStream_t stream)
{
    return launch<kMad>(matrix_dev, dtype, K, n, row_stride, DispersionArgs{0, 0, 0.0, 0.0}, scores_dev, stream);
}

int launch_percentile_range(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int index_lo, double g_lo,
                            int index_hi, double g_hi, double *scores_dev, hipStream_t stream)
{
    return launch<kIqr>(matrix_dev, dtype, K, n, row_stride, DispersionArgs{index_lo, index_hi, g_lo, g_hi}, scores_dev, stream);
}

int launch_std(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int pairwise_order, double *scores_dev,
               hipStream_t stream)
{
    if (!pairwise_order) {
        return launch<kStd>(matrix_dev, dtype, K, n, row_stride, DispersionArgs{0, 0, 0.0, 0.0}, scores_dev, stream);
    }
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    if (K > (size_t)kPairwiseMax) {
        return ROCCO_HIP_EINVAL;
    }
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dtype == 0) {
        hipLaunchKernelGGL((std_loop_kernel<double, true>), grid, block, 0, stream, (const double *)matrix_dev, (int)K, (long long)n,
                           (long long)row_stride, scores_dev);
    } else {
        hipLaunchKernelGGL((std_loop_kernel<float, true>), grid, block, 0, stream, (const float *)matrix_dev, (int)K, (long long)n,
                           (long long)row_stride, scores_dev);
    }
    ROCCO_HIP_TRY(hipGetLastError());
    return ROCCO_HIP_OK;
}

int launch_trimmed_std(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int rank_lo, int rank_hi,
                       int take_root, double *scores_dev, hipStream_t stream)
{
    return launch<kTstd>(matrix_dev, dtype, K, n, row_stride, DispersionArgs{rank_lo, rank_hi, take_root ? 1.0 : 0.0, 0.0}, scores_dev,
                         stream);
}

}  // namespace rocco
