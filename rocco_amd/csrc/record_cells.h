// rocco_amd/csrc/record_cells.h -- the per-record rule of ccounts_countRegion's alignment branch
// (rocco/native/ccounts_backend.c:2420-2560), shared by count.hip (bins of one region per track) and interval_count.hip
// (one bin per interval): one copy of the filter / fragment / clip / index arithmetic.
#pragma once

#include "../../include/rocco_hip.h"

namespace rocco {

namespace {

enum : int { kPaired = 1, kProperPair = 2, kUnmapped = 4, kMateUnmapped = 8, kReverse = 16, kRead2 = 128 };

// what a workgroup needs of its track
struct CountTrack {
    long long rec_begin, rec_end;  // its records in the concatenated arrays
    long long out_offset;          // its counts in the output buffer (floats)
    long long delta_offset;        // its difference array in the scratch (ints, n_bins + 1 cells)
    long long read_length, extend_bp, min_template_length, max_insert_size, shift_fwd, shift_rev;
    int start, end, step, n_bins;
    int flag_include, flag_exclude, min_mapq, paired_end_mode, one_read_per_bin;
    int pad_;
};

// The caller's options as the kernels read them, one conversion for count.hip and interval_count.hip: the two count the
// same record alike.  Records, region and buffer places are zero: the caller's to fill.
inline CountTrack count_track_from_options(const rocco_hip_count_options &o)
{
    CountTrack t = {};
    t.read_length = o.read_length;
    t.extend_bp = o.extend_bp;
    t.min_template_length = o.min_template_length;
    t.max_insert_size = o.max_insert_size;
    t.shift_fwd = o.shift_fwd;
    t.shift_rev = o.shift_rev;
    t.flag_include = o.flag_include > 0 ? (o.flag_include & 0xffff) : 0;  // uint16 in ccounts_countOptions
    t.flag_exclude = o.flag_exclude > 0 ? (o.flag_exclude & 0xffff) : 0;
    t.min_mapq = o.min_mapq;
    t.paired_end_mode = o.paired_end_mode;
    t.one_read_per_bin = o.one_read_per_bin != 0;
    return t;
}

// One record through the reference's loop (ccounts_backend.c:2420-2560).  Returns false when the record adds nothing;
// otherwise *i0 is the cell that gains one and *i1 the cell that loses one (-1: none, the one-read-per-bin form).
__device__ __forceinline__ bool record_cells(const CountTrack &t, long long pos, long long end, long long isize, int flag,
                                             int mapq, int mate_same, int *i0, int *i1)
{
    const long long start64 = t.start, end64 = t.end, step64 = t.step;
    // the index iterator yields only records that overlap the region as they lie in the file (before any shift or
    // extension): sam_itr_queryi(start, end) at :2400
    const long long it_end = end > pos + 1 ? end : pos + 1;
    if (!(pos < end64 && it_end > start64)) {
        return false;
    }
    if (t.flag_include > 0 && (flag & t.flag_include) != t.flag_include) {  // :2422
        return false;
    }
    if ((flag & t.flag_exclude) != 0) {  // :2427
        return false;
    }
    if (mapq < t.min_mapq) {  // :2431
        return false;
    }
    const long long read_start = pos, read_end = end;
    long long adj_start, adj_end;
    if (t.paired_end_mode > 0) {  // :2439-2487
        if ((flag & kProperPair) == 0 || (flag & kRead2) != 0 || (flag & kMateUnmapped) != 0 || !mate_same) {
            return false;
        }
        const long long min_template = t.min_template_length >= 0 ? t.min_template_length : t.read_length;  // :2416
        const long long abs_template = isize >= 0 ? isize : -isize;
        if (abs_template == 0 || abs_template < min_template) {
            return false;
        }
        if (t.max_insert_size > 0 && abs_template > t.max_insert_size) {
            return false;
        }
        if (isize >= 0) {
            adj_start = read_start;
            adj_end = read_start + abs_template;
        } else {
            adj_end = read_end;
            adj_start = adj_end - abs_template;
        }
        const long long shift = (flag & kReverse) == 0 ? t.shift_fwd : -t.shift_rev;
        adj_start += shift;
        adj_end += shift;
    } else if ((flag & kReverse) == 0) {  // :2490-2503
        if (t.extend_bp > 0) {
            adj_start = read_start + t.shift_fwd;
            adj_end = adj_start + t.extend_bp;
        } else {
            adj_start = read_start + t.shift_fwd;
            adj_end = read_end + t.shift_fwd;
        }
    } else {  // :2504-2517
        if (t.extend_bp > 0) {
            adj_end = (read_end - 1) - t.shift_rev + 1;
            adj_start = adj_end - t.extend_bp;
        } else {
            adj_start = read_start - t.shift_rev;
            adj_end = read_end - t.shift_rev;
        }
    }
    if (adj_end <= start64 || adj_start >= end64) {  // :2520
        return false;
    }
    if (adj_start < start64) {
        adj_start = start64;
    }
    if (adj_end > end64) {
        adj_end = end64;
    }
    const unsigned long long length = (unsigned long long)t.n_bins;
    if (t.one_read_per_bin) {  // :2533-2542
        const long long mid = (adj_start + adj_end) / 2;
        const unsigned long long index = (unsigned long long)((mid - start64) / step64);
        if (index >= length) {
            return false;
        }
        *i0 = (int)index;
        *i1 = -1;
        return true;
    }
    // (size_t) of a signed quotient, as the reference computes it (:2544-2557)
    const unsigned long long index0 = (unsigned long long)((adj_start - start64) / step64);
    unsigned long long index1 = (unsigned long long)(((adj_end - 1) - start64) / step64);
    if (index0 >= length) {
        return false;
    }
    if (index1 >= length) {
        index1 = length - 1;
    }
    if (index0 > index1) {
        return false;
    }
    *i0 = (int)index0;
    *i1 = (int)(index1 + 1);  // <= n_bins: the difference array has n_bins + 1 cells
    return true;
}

}  // namespace

}  // namespace rocco
