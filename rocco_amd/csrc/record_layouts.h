// rocco_amd/csrc/record_layouts.h -- where the launchers of count.hip, interval_count.hip, fragment_length.hip and
// bam_records.hip keep their regions of the solver's scratch buffer: one struct per launcher, read by its *_scratch_bytes (the total) and by
// the launcher itself (the offsets), so the two cannot drift apart.  A hipcub region takes the bytes hipcub asked for and
// is never empty.  Plain C++ (no HIP call): tests/host_logic/harness.cpp checks the layouts on the CPU.
#pragma once

#include "common.h"
#include "record_cells.h"

namespace rocco {

namespace {  // (as record_cells.h, whose CountTrack CountLayout measures)

// a track's difference array (n_bins + 1 cells, a multiple of 4) and its scan tiles
inline size_t count_delta_cells(size_t n_bins) { return (n_bins + 1 + 3) / 4 * 4; }
inline size_t count_scan_tiles(size_t n_bins) { return (n_bins + ROCCO_COUNT_SCAN_TILE - 1) / ROCCO_COUNT_SCAN_TILE; }

// launch_count_alignment_records: K tracks with `tiles` scan tiles and `cells` difference cells in all.  maxima, tile_sums
// and delta stay the tail of the buffer, in this order: the launcher zeroes them with one memset from `maxima` to `bytes`.
struct CountLayout {
    size_t tracks, chunk_first, tile_first, maxima, tile_sums, delta, bytes;
    CountLayout(size_t K, size_t tiles, size_t cells)
    {
        Layout lay;
        tracks = lay.at(K * sizeof(CountTrack));
        chunk_first = lay.at((K + 1) * sizeof(int));
        tile_first = lay.at((K + 1) * sizeof(int));
        maxima = lay.at(K * sizeof(int));
        tile_sums = lay.at(tiles * sizeof(int));
        delta = lay.at(cells * sizeof(int));
        bytes = lay.bytes();
    }
};

// launch_alignment_chrom_range_batch: the K + 1 record offsets and unit offsets, per track the first / last index, the 2 K
// values that go back
struct RangeBatchLayout {
    size_t rec_offsets, unit_first, first, last, range, bytes;
    explicit RangeBatchLayout(size_t K)
    {
        Layout lay;
        rec_offsets = lay.at((K + 1) * sizeof(long long));
        unit_first = lay.at((K + 1) * sizeof(long long));
        first = lay.at(K * sizeof(unsigned long long));
        last = lay.at(K * sizeof(unsigned long long));
        range = lay.at(2 * K * sizeof(long long));
        bytes = lay.bytes();
    }
};

// a track of track_supports_kernel: where its counts lie in the counter's output, how many, its file's norm_scale
struct SupportTrack {
    long long counts_offset, n_bins;
    double norm_scale;
};

// launch_track_supports, behind the counter's own layout: the tracks, their K + 1 unit offsets, per track first / last
struct SupportsLayout {
    size_t tracks, unit_first, first, last, bytes;
    explicit SupportsLayout(size_t K)
    {
        Layout lay;
        tracks = lay.at(K * sizeof(SupportTrack));
        unit_first = lay.at((K + 1) * sizeof(long long));
        first = lay.at(K * sizeof(unsigned long long));
        last = lay.at(K * sizeof(unsigned long long));
        bytes = lay.bytes();
    }
};

// launch_count_alignment_intervals: T tracks, `pairs` (interval, file) pairs, hipcub's scan over pairs + 1 unit counts
struct IntervalLayout {
    size_t rec_offsets, facts, cand_lo, cand_n, units, unit_first, scan, bytes;
    IntervalLayout(size_t T, size_t pairs, size_t scan_bytes)
    {
        Layout lay;
        rec_offsets = lay.at((T + 1) * sizeof(long long));
        facts = lay.at(2 * T * sizeof(int));
        cand_lo = lay.at(pairs * sizeof(long long));
        cand_n = lay.at(pairs * sizeof(int));
        units = lay.at((pairs + 1) * sizeof(long long));
        unit_first = lay.at((pairs + 1) * sizeof(long long));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

// launch_count_alignment_intervals_sets: IntervalLayout with one more int behind the 2 T facts, the call's error flag, so
// that facts and flag come back in one copy
struct IntervalSetsLayout {
    size_t rec_offsets, facts, cand_lo, cand_n, units, unit_first, scan, bytes;
    IntervalSetsLayout(size_t T, size_t pairs, size_t scan_bytes)
    {
        Layout lay;
        rec_offsets = lay.at((T + 1) * sizeof(long long));
        facts = lay.at((2 * T + 1) * sizeof(int));
        cand_lo = lay.at(pairs * sizeof(long long));
        cand_n = lay.at(pairs * sizeof(int));
        units = lay.at((pairs + 1) * sizeof(long long));
        unit_first = lay.at((pairs + 1) * sizeof(long long));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

// launch_record_flag_facts
struct FlagFactsLayout {
    size_t rec_offsets, mapped, unsorted, bytes;
    explicit FlagFactsLayout(size_t T)
    {
        Layout lay;
        rec_offsets = lay.at((T + 1) * sizeof(long long));
        mapped = lay.at(T * sizeof(unsigned long long));
        unsorted = lay.at(T * sizeof(int));
        bytes = lay.bytes();
    }
};

// launch_fragment_block_centers: six arrays of max_chunks + 1 cells (the longest contig's), hipcub's scan and sort
struct CentersLayout {
    size_t raw, prefix, density, index, density_sorted, index_sorted, cub, bytes;
    CentersLayout(size_t max_chunks, size_t cub_bytes)
    {
        const size_t cells = (max_chunks + 1) * sizeof(int);
        Layout lay;
        raw = lay.at(cells);
        prefix = lay.at(cells);
        density = lay.at(cells);
        index = lay.at(cells);
        density_sorted = lay.at(cells);
        index_sorted = lay.at(cells);
        cub = lay.at(cub_bytes > 0 ? cub_bytes : 1);
        bytes = lay.bytes();
    }
};

// launch_strand_xcorr_blocks
struct XcorrLayout {
    size_t rec_offsets, min_lag, block_track, block_start, best_lag, fwd_sum, rev_sum, best_score, bytes;
    XcorrLayout(size_t T, size_t n_blocks)
    {
        Layout lay;
        rec_offsets = lay.at((T + 1) * sizeof(long long));
        min_lag = lay.at(T * sizeof(int));
        block_track = lay.at(n_blocks * sizeof(int));
        block_start = lay.at(n_blocks * sizeof(long long));
        best_lag = lay.at(n_blocks * sizeof(int));
        fwd_sum = lay.at(n_blocks * sizeof(int));
        rev_sum = lay.at(n_blocks * sizeof(int));
        best_score = lay.at(n_blocks * sizeof(double));
        bytes = lay.bytes();
    }
};

// launch_template_lengths: hipcub's stream compaction over the longest track
struct TemplateLayout {
    size_t rec_offsets, min_insert, counts, select, bytes;
    TemplateLayout(size_t T, size_t select_bytes)
    {
        Layout lay;
        rec_offsets = lay.at((T + 1) * sizeof(long long));
        min_insert = lay.at(T * sizeof(int));
        counts = lay.at(T * sizeof(int));
        select = lay.at(select_bytes > 0 ? select_bytes : 1);
        bytes = lay.bytes();
    }
};

// segments of a stream of n_bytes (at least one: an empty stream is one empty segment)
inline size_t bam_walk_segments(size_t n_bytes, size_t segment_bytes)
{
    const size_t n = (n_bytes + segment_bytes - 1) / segment_bytes;
    return n > 0 ? n : 1;
}

// launch_bam_walk_records: per segment its entry, exit, count and the prefix sum of the counts (int64), why its walk
// stopped (int32); the report; hipcub's scan over the counts
struct BamWalkLayout {
    size_t entry, exit_of, count, first, stop, report, scan, bytes;
    BamWalkLayout(size_t n_segments, size_t scan_bytes)
    {
        Layout lay;
        entry = lay.at(n_segments * sizeof(long long));
        exit_of = lay.at(n_segments * sizeof(long long));
        count = lay.at(n_segments * sizeof(long long));
        first = lay.at(n_segments * sizeof(long long));
        stop = lay.at(n_segments * sizeof(int));
        report = lay.at(ROCCO_BAM_WALK_REPORT * sizeof(long long));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

// launch_bam_record_fields: the n_ref + 2 contig offsets and the error word
struct BamFieldsLayout {
    size_t contig_first, error, bytes;
    explicit BamFieldsLayout(size_t n_ref)
    {
        Layout lay;
        contig_first = lay.at((n_ref + 2) * sizeof(long long));
        error = lay.at(sizeof(unsigned long long));
        bytes = lay.bytes();
    }
};

// launch_bam_stream_firsts: the K + 1 bounds and the K + 1 first records (int64), the K expected reference ids (int32), the
// error word
struct BamStreamFirstsLayout {
    size_t bound, firsts, expect, error, bytes;
    explicit BamStreamFirstsLayout(size_t K)
    {
        Layout lay;
        bound = lay.at((K + 1) * sizeof(long long));
        firsts = lay.at((K + 1) * sizeof(long long));
        expect = lay.at((K > 0 ? K : 1) * sizeof(int));
        error = lay.at(sizeof(unsigned long long));
        bytes = lay.bytes();
    }
};

// launch_inflate: per block its status (int32) and the bytes it inflates to (int64), each unused where the caller brings its
// own; with_ends (zlib framing): per block where its stream ended in the compressed buffer (int64); the word of the first
// failing block; the report
struct InflateLayout {
    size_t status, produced, ends = 0, first_error, report, bytes;
    InflateLayout(size_t n_blocks, bool with_ends)
    {
        Layout lay;
        status = lay.at(n_blocks * sizeof(int));
        produced = lay.at(n_blocks * sizeof(long long));
        if (with_ends) {
            ends = lay.at(n_blocks * sizeof(long long));
        }
        first_error = lay.at(sizeof(unsigned long long));
        report = lay.at(ROCCO_BGZF_REPORT * sizeof(long long));
        bytes = lay.bytes();
    }
};

// launch_bigwig_sections_facts / _emit: the files' arrays as they go up (n_files + 1 block offsets, n_files chromosome ids,
// n_files chromosome lengths, int64; first, so that both calls find them at one place whatever hipcub asks for), the
// n_blocks + 1 kept-item counts (int64), the word of the first refused block, what comes back (the report and the
// n_files + 1 interval offsets, int64), hipcub's scan over the counts
struct SectionsLayout {
    size_t files, counts, first_error, back, scan, bytes;
    SectionsLayout(size_t n_blocks, size_t n_files, size_t scan_bytes)
    {
        Layout lay;
        files = lay.at((3 * n_files + 1) * sizeof(long long));
        counts = lay.at((n_blocks + 1) * sizeof(long long));
        first_error = lay.at(sizeof(unsigned long long));
        back = lay.at((ROCCO_BGZF_REPORT + n_files + 1) * sizeof(long long));
        scan = lay.at(scan_bytes > 0 ? scan_bytes : 1);
        bytes = lay.bytes();
    }
};

}  // namespace

}  // namespace rocco
