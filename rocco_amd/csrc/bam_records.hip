// rocco_amd/csrc/bam_records.hip -- the inflated bytes of a BAM file -> record offsets -> the arrays rows f5-f7 consume
// (note (29)), gfx950.
//
// Replaces what the reference's counter has htslib do per record (rocco/native/ccounts_backend.c reads through
// sam_itr_next / sam_read1):
//   bam_read1       the record framing (block_size, the 32 fixed bytes, its consistency checks)   bam_guess_kernel,
//                                                                                                  bam_walk_kernel,
//                                                                                                  bam_stitch_kernel,
//                                                                                                  bam_emit_kernel
//   bam_endpos      pos + reference length of the CIGAR (0 for an unmapped record; 0 becomes 1)    bam_fields_kernel
//   bam_cigar2qlen  the query length of the CIGAR where l_seq <= 0                                 bam_fields_kernel
// BGZF inflate is the host's (rocco_amd/bam.py) or bgzf_inflate.hip's; bam_tag2cigar (the CG tag) is not decoded: it is reported.
//
// The record stream is a linked list: a record's first word says where the next begins.  It is cut into segments of S
// bytes.  Every segment i guesses its entry (the lowest offset in [iS, (i + 1)S) from which kBamGuessDepth records in a row
// are plausible, bam_record.h), all segments are walked from their guesses in parallel, then ONE wavefront follows the
// true chain from entry0 across the per-segment results: a segment whose guess equals the exit of the last confirmed
// segment is confirmed as it stands; one whose guess differs is walked again from the true entry, there and then; a
// segment the chain jumps over (a record longer than S) is overruled to "none".  By induction from entry0 every
// confirmed entry is a true record start, so the output is the sequential walk's whatever was guessed; the guesses only
// decide how much of the walk ran in parallel.  A stop noted by a walk that is not confirmed is dropped with the walk.
#include "kernels.h"
#include "bam_record.h"
#include "record_layouts.h"
#include "record_stream.h"

#include <hipcub/hipcub.hpp>

#include <vector>

namespace rocco {

namespace {

constexpr int kThreads = ROCCO_BAM_THREADS;
constexpr int kWave = 64;
constexpr int kMaxGrid = ROCCO_BAM_MAX_GRID;  // workgroups of a launch at most
constexpr long long kNone = -1;

static_assert(kThreads == 256 && kBamGuessDepth >= 1 && kMaxGrid > 0, "rocco_hip.h states the shape");

unsigned bam_grid_for(long long items, int per_group)
{
    const long long groups = (items + per_group - 1) / per_group;
    return (unsigned)(groups < 1 ? 1 : (groups > kMaxGrid ? kMaxGrid : groups));
}

// entry[i]: the guess of segment i.  Segments before entry0's have none, entry0's has entry0.  One workgroup per segment (grid
// stride); a tile of kThreads candidates and the 35 bytes behind it are staged in LDS, every lane tests one candidate.
__global__ __launch_bounds__(kThreads) void bam_guess_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, long long entry0,
                                                            int n_ref, int shift, long long n_segments, int guess_mode,
                                                            long long *__restrict__ entry)
{
    __shared__ uint8_t tile[kThreads + kBamFixed];
    __shared__ int best;
    const long long seg0 = entry0 >> shift;
    for (long long i = blockIdx.x; i < n_segments; i += gridDim.x) {
        const long long lo = i << shift, hi = lo + (1LL << shift);
        if (i <= seg0 || guess_mode == 0) {
            if (threadIdx.x == 0) {
                entry[i] = i < seg0 ? kNone : (i == seg0 ? entry0 : lo);
            }
            continue;
        }
        long long found = kNone;
        const long long last = (hi < n_bytes - kBamFixed + 1) ? hi : n_bytes - kBamFixed + 1;  // candidates lie in [lo, last)
        for (long long base = lo; base < last; base += kThreads) {  // (uniform over the workgroup)
            __syncthreads();
            if (threadIdx.x == 0) {
                best = kThreads;
            }
            for (int k = threadIdx.x; k < kThreads + kBamFixed; k += kThreads) {
                tile[k] = base + k < n_bytes ? bytes[base + k] : (uint8_t)0;
            }
            __syncthreads();
            const long long o = base + threadIdx.x;
            if (o < last && bam_plausible_chain(bytes, n_bytes, o, n_ref, tile, threadIdx.x)) {
                atomicMin(&best, (int)threadIdx.x);
            }
            __syncthreads();
            if (best < kThreads) {
                found = base + best;
                break;
            }
        }
        if (threadIdx.x == 0) {
            entry[i] = found;
        }
    }
}

// one lane per segment: the walk from its guess
__global__ __launch_bounds__(kThreads) void bam_walk_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, int shift,
                                                           long long n_segments, const long long *__restrict__ entry,
                                                           long long *__restrict__ exit_of, long long *__restrict__ count,
                                                           int *__restrict__ stop)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_segments; i += (long long)gridDim.x * kThreads) {
        const long long p = entry[i];
        long long n = 0, x = kNone;
        int why = kBamStopNone;
        if (p >= 0) {
            x = bam_walk_segment<false>(bytes, n_bytes, p, (i + 1) << shift, nullptr, 0, &n, &why);
        }
        exit_of[i] = x;
        count[i] = n;
        stop[i] = why;
    }
}

// One wavefront follows the true chain over the segments' results, 64 segments per load; every lane holds the same chain
// state, lane k the results of segment base + k.  A wrong guess is repaired on the spot: the wavefront walks the segment
// from its true entry (all lanes the same loads).  Leaves entry[i] = the confirmed entry or none, count[i] = its starts.
// report: [0] records, [1] the offset behind the last complete record, [2] segments, [3] wrong guesses, [4] segments
// walked again, [5] why the chain stopped (0: at n_bytes exactly), [6] where
__global__ __launch_bounds__(kWave) void bam_stitch_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, long long entry0,
                                                          int shift, long long n_segments, long long *__restrict__ entry,
                                                          const long long *__restrict__ exit_of, long long *__restrict__ count,
                                                          const int *__restrict__ stop, long long *__restrict__ report)
{
    const int lane = threadIdx.x;
    long long cur = entry0, records = 0, wrong = 0, repairs = 0;
    int stopped = kBamStopNone;
    for (long long base = 0; base < n_segments; base += kWave) {
        const long long i = base + lane;
        const bool have = i < n_segments;
        long long g = have ? entry[i] : kNone, x = have ? exit_of[i] : kNone, c = have ? count[i] : 0;
        int s = have ? stop[i] : 0;
        const int m = n_segments - base < kWave ? (int)(n_segments - base) : kWave;
        for (int k = 0; k < m; ++k) {
            const long long gk = __shfl(g, k);
            long long xk = __shfl(x, k), ck = __shfl(c, k);
            int sk = __shfl(s, k);
            const long long lo = (base + k) << shift, hi = lo + (1LL << shift);
            const bool alive = stopped == kBamStopNone && cur < n_bytes;
            if (alive && cur >= lo && cur < hi) {
                if (gk != cur) {
                    ++wrong;
                    ++repairs;
                    xk = bam_walk_segment<false>(bytes, n_bytes, cur, hi, nullptr, 0, &ck, &sk);
                    if (lane == k) {
                        g = cur;
                        c = ck;
                    }
                }
                records += ck;
                cur = xk;
                stopped = sk;
            } else if (gk >= 0) {
                wrong += alive ? 1 : 0;  // (behind the chain's end nothing is guessed wrongly: there is no truth left)
                if (lane == k) {
                    g = kNone;
                    c = 0;
                }
            }
        }
        if (have) {
            entry[i] = g;
            count[i] = c;
        }
    }
    if (lane == 0) {
        report[0] = records;
        report[1] = cur;
        report[2] = n_segments;
        report[3] = wrong;
        report[4] = repairs;
        report[5] = stopped != kBamStopNone ? stopped : (cur == n_bytes ? 0 : ROCCO_BAM_ERR_TRUNCATED);
        report[6] = stopped != kBamStopNone || cur != n_bytes ? cur : -1;
    }
}

// one lane per confirmed segment: its walk again, storing the starts behind the prefix sum of the counts
__global__ __launch_bounds__(kThreads) void bam_emit_kernel(const uint8_t *__restrict__ bytes, long long n_bytes, int shift,
                                                           long long n_segments, const long long *__restrict__ entry,
                                                           const long long *__restrict__ first, long long *__restrict__ offsets_out,
                                                           long long capacity)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_segments; i += (long long)gridDim.x * kThreads) {
        const long long p = entry[i], at = first[i];
        if (p >= 0 && at < capacity) {
            long long n;
            int why;
            (void)bam_walk_segment<true>(bytes, n_bytes, p, (i + 1) << shift, offsets_out + at, capacity - at, &n, &why);
        }
    }
}

__device__ __forceinline__ void note_error(unsigned long long *error, long long record, int code)
{
    atomicMin(error, ((unsigned long long)record << 8) | (unsigned long long)code);
}

// one lane per record.  error: the lowest (record << 8 | code) seen.
__global__ __launch_bounds__(kThreads) void bam_fields_kernel(const uint8_t *__restrict__ bytes, long long n_bytes,
                                                             const long long *__restrict__ offsets, long long n, int n_ref,
                                                             int *__restrict__ tid_out, int *__restrict__ pos_out,
                                                             int *__restrict__ end_out, int *__restrict__ isize_out,
                                                             unsigned short *__restrict__ flag_out, uint8_t *__restrict__ mapq_out,
                                                             uint8_t *__restrict__ mate_same_out, int *__restrict__ qlen_out,
                                                             unsigned long long *__restrict__ error)
{
    for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < n; r += (long long)gridDim.x * kThreads) {
        const long long p = offsets[r];
        int tid = -1, pos = -1, end = 0, isize = 0, qlen = 0;
        unsigned flag = 4, mapq = 0, mate_same = 0;
        bool framed = p >= 0 && p + kBamFixed <= n_bytes;
        long long block_size = 0;
        if (framed) {
            block_size = bam_i32(bytes, p);
            framed = block_size >= kBamMinBlockSize && p + 4 + block_size <= n_bytes;
        }
        if (!framed) {
            note_error(error, r, ROCCO_BAM_ERR_OFFSET);
        } else {
            tid = bam_i32(bytes, p + 4);
            pos = bam_i32(bytes, p + 8);
            const long long l_read_name = bam_u8(bytes, p + 12), n_cigar = bam_u16(bytes, p + 16), l_seq = bam_i32(bytes, p + 20);
            mapq = bam_u8(bytes, p + 13);
            flag = bam_u16(bytes, p + 18);
            const int mtid = bam_i32(bytes, p + 24);
            isize = bam_i32(bytes, p + 32);
            mate_same = mtid == tid ? 1u : 0u;
            const bool sizes_ok = l_seq >= 0 && 4 * n_cigar + l_read_name + (l_seq + 1) / 2 + l_seq <= block_size - kBamMinBlockSize;
            if (!sizes_ok) {
                note_error(error, r, ROCCO_BAM_ERR_SIZES);
            }
            if (l_read_name < 1) {
                note_error(error, r, ROCCO_BAM_ERR_READ_NAME);
            }
            if (tid < -1 || tid >= n_ref || mtid < -1 || mtid >= n_ref) {
                note_error(error, r, ROCCO_BAM_ERR_REF_ID);
            }
            if (tid >= 0 && pos < 0) {
                note_error(error, r, ROCCO_BAM_ERR_POSITION);
            }
            long long rlen = 0, cigar_qlen = 0;
            if (sizes_ok) {  // (the CIGAR lies inside the record, the record inside the stream)
                const long long cigar = p + kBamFixed + l_read_name;
                for (long long k = 0; k < n_cigar; ++k) {
                    const unsigned word = bam_u32(bytes, cigar + 4 * k);
                    const unsigned op = word & 15u;
                    const long long len = word >> 4;
                    // M I D N S H P = X: 0 .. 8.  reference: M D N = X; query: M I S = X
                    rlen += ((0x18Du >> op) & 1u) ? len : 0;
                    cigar_qlen += ((0x193u >> op) & 1u) ? len : 0;
                }
                if (n_cigar > 0) {
                    const unsigned word = bam_u32(bytes, cigar);
                    if (tid >= 0 && pos >= 0 && (word & 15u) == 4u && (long long)(word >> 4) == l_seq) {
                        note_error(error, r, ROCCO_BAM_ERR_CG_TAG);
                    }
                    if ((flag & 4u) == 0 && l_seq > 0 && cigar_qlen != l_seq) {
                        note_error(error, r, ROCCO_BAM_ERR_CIGAR_SEQ);
                    }
                }
            }
            if (flag & 4u) {
                rlen = 0;
            }
            const long long e = (long long)pos + (rlen == 0 ? 1 : rlen);
            if (e >= (1LL << 31)) {
                note_error(error, r, ROCCO_BAM_ERR_END);
            }
            end = (int)(e < (1LL << 31) ? e : 0x7fffffff);
            const long long q = (l_seq <= 0 && n_cigar > 0) ? cigar_qlen : l_seq;
            qlen = (int)(q < 0x7fffffffLL ? q : 0x7fffffffLL);
            if (r > 0) {  // file order of a coordinate-sorted BAM: tid ascends, the records without a contig come last
                const long long before = offsets[r - 1];
                if (before >= 0 && before + kBamFixed <= n_bytes) {
                    const int t0 = bam_i32(bytes, before + 4);
                    const long long k0 = t0 < 0 ? n_ref : t0, k1 = tid < 0 ? n_ref : tid;
                    if (k0 > k1) {
                        note_error(error, r, ROCCO_BAM_ERR_ORDER);
                    }
                }
            }
        }
        tid_out[r] = tid;
        pos_out[r] = pos;
        end_out[r] = end;
        isize_out[r] = isize;
        flag_out[r] = (unsigned short)flag;
        mapq_out[r] = (uint8_t)mapq;
        mate_same_out[r] = (uint8_t)mate_same;
        qlen_out[r] = qlen;
    }
}

// contig_first[k], k = 0 .. n_ref: the first record whose contig is k or later (the records without one count as n_ref);
// contig_first[n_ref + 1] = n.  A bisection per contig over an ascending tid.
__global__ __launch_bounds__(kThreads) void bam_contig_first_kernel(const int *__restrict__ tid, long long n, int n_ref,
                                                                   long long *__restrict__ contig_first)
{
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k <= (long long)n_ref + 1; k += (long long)gridDim.x * kThreads) {
        long long lo = 0, hi = n;
        while (lo < hi && k <= n_ref) {
            const long long mid = lo + ((hi - lo) >> 1);
            const int t = tid[mid];
            if ((t < 0 ? (long long)n_ref : (long long)t) < k) {
                lo = mid + 1;
            } else {
                hi = mid;
            }
        }
        contig_first[k] = k <= n_ref ? lo : n;
    }
}

// One lane per record of a chain walked over K streams laid one behind the other (rocco_amd/bam.py: read_alignment_spans):
// bound[j], j = 0 .. K, are the ascending byte bounds of the streams (an empty stream repeats a bound, bound[K] = n_bytes).
// Record r at offset o belongs to stream s = (the number of j in [0, K] with bound[j] <= o) - 1, the upper bound, so that
// among repeated bounds the last one takes the record and the streams before it stay empty.  firsts[j]: the first record at
// or after bound[j] (n where there is none).  The first record of its stream writes firsts[j] for every j behind the
// stream of the record before it, the last record writes those behind its own: every firsts[j] is written once.
// error: the lowest (stream << 8 | code) seen.
__global__ __launch_bounds__(kThreads) void bam_stream_firsts_kernel(const long long *__restrict__ offsets, const int *__restrict__ tid,
                                                                    long long n, const long long *__restrict__ bound,
                                                                    const int *__restrict__ expect_tid, int K,
                                                                    long long *__restrict__ firsts, unsigned long long *__restrict__ error)
{
    const long long stride = (long long)gridDim.x * kThreads;
    const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n == 0) {
        for (long long j = lane; j <= K; j += stride) {
            firsts[j] = 0;
        }
        return;
    }
    for (long long r = lane; r < n; r += stride) {
        const long long o = offsets[r];
        // s: the last j in [0, K) with bound[j] <= o (0 where o lies in front of bound[0]: a seam error below)
        int lo = 0, hi = K;  // the count of j in [0, K) with bound[j] <= o lies in [lo, hi]
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (bound[mid] <= o) {
                lo = mid + 1;
            } else {
                hi = mid;
            }
        }
        const int s = lo > 0 ? lo - 1 : 0;
        int before = -1;  // the stream of the record in front (-1: none)
        if (r > 0) {
            const long long o0 = offsets[r - 1];
            int lo0 = 0, hi0 = s + 1;  // (offsets ascend: it is no later than s)
            while (lo0 < hi0) {
                const int mid = lo0 + ((hi0 - lo0) >> 1);
                if (bound[mid] <= o0) {
                    lo0 = mid + 1;
                } else {
                    hi0 = mid;
                }
            }
            before = lo0 > 0 ? lo0 - 1 : 0;
        }
        if (before < s) {  // the first record of stream s: every bound passed since the record in front must lie on it
            if (o != bound[before + 1]) {
                note_error(error, before + 1, ROCCO_BAM_ERR_SEAM);
            }
            for (int j = before + 1; j <= s; ++j) {
                firsts[j] = r;
            }
        }
        if (tid[r] != expect_tid[s]) {
            note_error(error, s, ROCCO_BAM_ERR_SPAN_TID);
        }
        if (r == n - 1) {
            if (o >= bound[K]) {
                note_error(error, s, ROCCO_BAM_ERR_SEAM);
            } else if (s + 1 < K && bound[s + 1] != bound[K]) {  // (bytes behind the last record that belong to a later stream)
                note_error(error, s + 1, ROCCO_BAM_ERR_SEAM);
            }
            for (int j = s + 1; j <= K; ++j) {
                firsts[j] = n;
            }
        }
    }
}

size_t walk_scan_bytes(size_t n_segments)
{
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const long long *)nullptr, (long long *)nullptr, (int)n_segments) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes > 0 ? bytes : 1;
}

int shift_of(size_t segment_bytes)
{
    int shift = 0;
    while (((size_t)1 << shift) < segment_bytes) {
        ++shift;
    }
    return shift;
}

}  // namespace

size_t bam_walk_scratch_bytes(size_t n_bytes, size_t segment_bytes)
{
    if (segment_bytes < 64 || (segment_bytes & (segment_bytes - 1)) != 0 || segment_bytes > ((size_t)1 << 30) ||
        n_bytes >= ((size_t)1 << 62)) {
        set_last_error("bam_walk_records: segment_bytes must be a power of two in [64, 2^30]");
        return 0;
    }
    const size_t n_segments = bam_walk_segments(n_bytes, segment_bytes);
    if (n_segments >= (size_t)0x7fffffff) {
        set_last_error("bam_walk_records: 2^31 segments or more; pass a shorter slab or a larger segment_bytes");
        return 0;
    }
    const size_t scan = walk_scan_bytes(n_segments);
    return scan == 0 ? 0 : BamWalkLayout(n_segments, scan).bytes;
}

int launch_bam_walk_records(const uint8_t *bytes_dev, size_t n_bytes, int64_t entry0, int n_ref, size_t segment_bytes, int guess_mode,
                            int64_t *offsets_out_dev, size_t capacity, int64_t *segment_entry_out_dev, int64_t *report_out_host,
                            void *scratch_dev, hipStream_t stream)
{
    const size_t n_segments = bam_walk_segments(n_bytes, segment_bytes);
    const int shift = shift_of(segment_bytes);
    const BamWalkLayout at(n_segments, walk_scan_bytes(n_segments));
    char *sc = (char *)scratch_dev;
    long long *entry = (long long *)(sc + at.entry), *exit_of = (long long *)(sc + at.exit_of), *count = (long long *)(sc + at.count);
    long long *first = (long long *)(sc + at.first), *report = (long long *)(sc + at.report);
    int *stop = (int *)(sc + at.stop);
    size_t scan_bytes = at.bytes - at.scan;
    long long back[ROCCO_BAM_WALK_REPORT] = {0};
    const int queued = queue_then_drain(stream, [&]() -> int {
        hipLaunchKernelGGL(bam_guess_kernel, dim3(bam_grid_for((long long)n_segments, 1)), dim3(kThreads), 0, stream, bytes_dev,
                           (long long)n_bytes, (long long)entry0, n_ref, shift, (long long)n_segments, guess_mode, entry);
        ROCCO_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bam_walk_kernel, dim3(bam_grid_for((long long)n_segments, kThreads)), dim3(kThreads), 0, stream, bytes_dev,
                           (long long)n_bytes, shift, (long long)n_segments, (const long long *)entry, exit_of, count, stop);
        ROCCO_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bam_stitch_kernel, dim3(1), dim3(kWave), 0, stream, bytes_dev, (long long)n_bytes, (long long)entry0, shift,
                           (long long)n_segments, entry, (const long long *)exit_of, count, (const int *)stop, report);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc + at.scan, scan_bytes, (const long long *)count, first, (int)n_segments, stream));
        hipLaunchKernelGGL(bam_emit_kernel, dim3(bam_grid_for((long long)n_segments, kThreads)), dim3(kThreads), 0, stream, bytes_dev,
                           (long long)n_bytes, shift, (long long)n_segments, (const long long *)entry, (const long long *)first,
                           (long long *)offsets_out_dev, (long long)capacity);
        ROCCO_HIP_TRY(hipGetLastError());
        if (segment_entry_out_dev != nullptr) {
            ROCCO_HIP_TRY(hipMemcpyAsync(segment_entry_out_dev, entry, n_segments * sizeof(long long), hipMemcpyDeviceToDevice, stream));
        }
        ROCCO_HIP_TRY(hipMemcpyAsync(back, report, sizeof(back), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (int k = 0; k < ROCCO_BAM_WALK_REPORT; ++k) {
        report_out_host[k] = back[k];
    }
    if (back[0] > (long long)capacity) {
        set_last_error("bam_walk_records: the stream holds " + std::to_string(back[0]) + " records, offsets_out_dev has room for " +
                       std::to_string(capacity) + " (n_bytes / 36 + 1 always suffices)");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

size_t bam_record_fields_scratch_bytes(int n_ref) { return n_ref < 0 ? 0 : BamFieldsLayout((size_t)n_ref).bytes; }

int launch_bam_record_fields(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *offsets_dev, size_t n, int n_ref, int32_t *tid_out_dev,
                             int32_t *pos_out_dev, int32_t *end_out_dev, int32_t *isize_out_dev, uint16_t *flag_out_dev,
                             uint8_t *mapq_out_dev, uint8_t *mate_same_out_dev, int32_t *qlen_out_dev, int64_t *contig_first_out_host,
                             int64_t *report_out_host, void *scratch_dev, hipStream_t stream)
{
    const BamFieldsLayout at((size_t)n_ref);
    char *sc = (char *)scratch_dev;
    long long *contig_first = (long long *)(sc + at.contig_first);
    unsigned long long *error = (unsigned long long *)(sc + at.error);
    std::vector<long long> firsts((size_t)n_ref + 2, 0);
    unsigned long long packed = ~0ULL;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemsetAsync(error, 0xff, sizeof(unsigned long long), stream));
        if (n > 0) {
            hipLaunchKernelGGL(bam_fields_kernel, dim3(bam_grid_for((long long)n, kThreads)), dim3(kThreads), 0, stream, bytes_dev,
                               (long long)n_bytes, (const long long *)offsets_dev, (long long)n, n_ref, tid_out_dev, pos_out_dev, end_out_dev,
                               isize_out_dev, (unsigned short *)flag_out_dev, mapq_out_dev, mate_same_out_dev, qlen_out_dev, error);
            ROCCO_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(bam_contig_first_kernel, dim3(bam_grid_for((long long)n_ref + 2, kThreads)), dim3(kThreads), 0, stream,
                           (const int *)tid_out_dev, (long long)n, n_ref, contig_first);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(firsts.data(), contig_first, firsts.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(&packed, error, sizeof(packed), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t k = 0; k < firsts.size(); ++k) {
        contig_first_out_host[k] = firsts[k];
    }
    report_out_host[0] = packed == ~0ULL ? 0 : (int64_t)(packed & 0xffULL);
    report_out_host[1] = packed == ~0ULL ? -1 : (int64_t)(packed >> 8);
    return ROCCO_HIP_OK;
}

size_t bam_stream_firsts_scratch_bytes(size_t K) { return BamStreamFirstsLayout(K).bytes; }

int launch_bam_stream_firsts(const int64_t *offsets_dev, const int32_t *tid_dev, size_t n, const int64_t *bounds_host,
                             const int32_t *expect_tid_host, size_t K, int64_t *firsts_out_host, int64_t *report_out_host, void *scratch_dev,
                             hipStream_t stream)
{
    const BamStreamFirstsLayout at(K);
    char *sc = (char *)scratch_dev;
    long long *bound = (long long *)(sc + at.bound), *firsts = (long long *)(sc + at.firsts);
    int *expect = (int *)(sc + at.expect);
    unsigned long long *error = (unsigned long long *)(sc + at.error);
    std::vector<long long> back(K + 1, 0);
    unsigned long long packed = ~0ULL;
    const int queued = queue_then_drain(stream, [&]() -> int {
        ROCCO_HIP_TRY(hipMemcpyAsync(bound, bounds_host, (K + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        if (K > 0) {
            ROCCO_HIP_TRY(hipMemcpyAsync(expect, expect_tid_host, K * sizeof(int), hipMemcpyHostToDevice, stream));
        }
        ROCCO_HIP_TRY(hipMemsetAsync(error, 0xff, sizeof(unsigned long long), stream));
        const long long items = n > K + 1 ? (long long)n : (long long)K + 1;
        hipLaunchKernelGGL(bam_stream_firsts_kernel, dim3(bam_grid_for(items, kThreads)), dim3(kThreads), 0, stream,
                           (const long long *)offsets_dev, (const int *)tid_dev, (long long)n, (const long long *)bound, (const int *)expect,
                           (int)K, firsts, error);
        ROCCO_HIP_TRY(hipGetLastError());
        ROCCO_HIP_TRY(hipMemcpyAsync(back.data(), firsts, back.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipMemcpyAsync(&packed, error, sizeof(packed), hipMemcpyDeviceToHost, stream));
        ROCCO_HIP_TRY(hipStreamSynchronize(stream));
        return ROCCO_HIP_OK;
    });
    if (queued != ROCCO_HIP_OK) {
        return queued;
    }
    for (size_t j = 0; j <= K; ++j) {
        firsts_out_host[j] = back[j];
    }
    report_out_host[0] = packed == ~0ULL ? 0 : (int64_t)(packed & 0xffULL);
    report_out_host[1] = packed == ~0ULL ? -1 : (int64_t)(packed >> 8);
    return ROCCO_HIP_OK;
}

}  // namespace rocco
