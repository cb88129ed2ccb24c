// rocco_amd/csrc/kernels.h -- device task descriptors and launchers shared by the .hip files.
#pragma once

#include "common.h"

namespace rocco {
#if defined(__HIPCC__)
// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wavefront's global loads and stores
// (s_waitcnt vmcnt(0)): a wavefront that has just issued the loads of a tile it needs three trips later then sits out a
// memory latency at every barrier -- measured in round 5 on the rolling-sums launch: 22 ns per locus with the chain AND the
// variances compiled out.  The tiles these kernels hand over live in LDS; what they read from or write to global memory
// is touched by one thread only.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
#endif


// ---- chain_exact.hip ------------------------------------------------------------------------
struct ExactTask {
    const double *scores;         // n
    const double *switch_costs;   // n-1 or nullptr
    double gamma;
    long long n;
    const double *lambdas;        // n_lambda penalties (device)
    int n_lambda;                 // 1..64
    int record_lane;              // lane whose decisions are recorded + backtracked
    double *values_out;           // n_lambda
    long long *counts_out;        // n_lambda
    unsigned long long *decision_words;  // ceil((n-1)/32) words or nullptr
    uint8_t *solution;            // n bytes (used iff decision_words)
};

int launch_chain_exact(const ExactTask *tasks_dev, int n_tasks, hipStream_t stream);

// ---- median.hip -----------------------------------------------------------------------------
int launch_median(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                  double *scores_dev, hipStream_t stream);

// several matrices of one K / element type in one launch (kernel-argument task table: up to kMedianBatchMax per launch)
constexpr int kMedianBatchMax = 48;
struct MedianTask {
    const void *matrix;
    double *out;
    long long n;
    long long stride;
    unsigned block_begin;
    unsigned pad;
    double *partials;  // [wavefront of this task][3] = min, max, sum |.| of its scores (nullptr: not wanted)
};
struct MedianBatch {
    // first workgroup of every task, ascending; unused slots hold 0xFFFFFFFF.  Kept apart from the task records so that
    // a workgroup finds its task with a few wide scalar loads and compares in registers -- not one dependent scalar
    // load per task before its first vector load can issue (24 chromosomes: 0.5 ms per genome launch)
    unsigned block_begin[kMedianBatchMax];
    MedianTask tasks[kMedianBatchMax];
    int n_tasks;
    int K;
};
// `stats_dev` (optional): [count][3] = min, max and sum of absolute values of every score array (what the budgeted
// solve otherwise reads the scores once more for), reduced from per-workgroup partials kept in `partials_dev`
// (3 doubles per 64 loci of every matrix; median_partials_count() tells how many wavefronts that is).
size_t median_partials_count(const size_t *n, size_t count);
int launch_median_batch(const void *const *matrices_dev, int dtype, size_t K, const size_t *n, const size_t *row_strides,
                        double *const *scores_dev, size_t count, hipStream_t stream, double *stats_dev = nullptr,
                        double *partials_dev = nullptr);

int launch_order_statistic(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int rank,
                           double *scores_dev, hipStream_t stream);
int launch_column_mean(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, double *scores_dev,
                       hipStream_t stream);
int launch_trimmed_mean(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int rank_lo, int rank_hi,
                        double *scores_dev, hipStream_t stream);
int launch_power(const double *x_dev, double p, double *out_dev, size_t n, hipStream_t stream);

// ---- dispersion.hip -------------------------------------------------------------------------
// column-wise dispersion of a [K][row_stride] matrix, 2 <= K (matrix conventions of launch_median)
int launch_mad(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, double *scores_dev, hipStream_t stream);
int launch_percentile_range(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int index_lo, double g_lo,
                            int index_hi, double g_hi, double *scores_dev, hipStream_t stream);
int launch_std(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int pairwise_order, double *scores_dev,
               hipStream_t stream);
int launch_trimmed_std(const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, int rank_lo, int rank_hi,
                       int take_root, double *scores_dev, hipStream_t stream);

// ---- select.hip -----------------------------------------------------------------------------
// order statistics of `count` vectors by a batched radix select, nothing n-long written (see the head of select.hip)
constexpr int kSelectBatchMax = 48;  // vectors per series of launches (kernel-argument task table); more are served group by group
constexpr int kSelectRanksMax = 16;  // ranks followed per vector
size_t select_scratch_bytes(size_t count);
// vectors_dev / n / centers: host arrays of `count` entries; ranks: host, [count][n_ranks], each below its n;
// values_out_dev: [count][n_ranks]; counts_out_dev: [count][4].  Everything is queued on `stream`, nothing is waited for.
int launch_select_ranks_batch(const double *const *vectors_dev, const size_t *n, size_t count, int n_ranks, const long long *ranks,
                              int mode, const double *centers, double *values_out_dev, long long *counts_out_dev, void *scratch_dev,
                              hipStream_t stream);
int launch_bh_last_passing_rank(const double *sorted_dev, size_t m, double fdr, long long *rank_out_dev, hipStream_t stream);
int launch_threshold_mask(const double *x_dev, size_t n, double divisor, double threshold, double floor_value, int use_floor,
                          uint8_t *mask_out_dev, hipStream_t stream);
int launch_at_most_mask(const double *x_dev, size_t n, double cutoff, uint8_t *mask_out_dev, hipStream_t stream);
int launch_divide_finite(const double *x_dev, size_t n, double divisor, double *out_dev, hipStream_t stream);

// ---- decode.hip -----------------------------------------------------------------------------
// scratch: at least decode_scratch_bytes(n) bytes
size_t decode_scratch_bytes(size_t n);
int launch_decode_runs(const uint8_t *solution_dev, size_t n, int64_t *run_begin_dev,
                       int64_t *run_end_dev, size_t capacity, void *scratch_dev,
                       unsigned long long *n_runs_host_pinned, hipStream_t stream);

// several solutions in three launches and one synchronisation (n <= 1 tasks must be left out by the caller)
constexpr int kDecodeBatchMax = 48;
struct DecodeTask {
    const uint8_t *solution;
    long long n;
    long long tile_begin;  // first tile of this task in the launches (decode_tiles(n) tiles each)
    int64_t *run_begin;    // (table form: the table itself, rows of 3 values)
    int64_t *run_end;      // (table form: unused)
    unsigned long long capacity;  // (table form: rows of the whole table)
    long long unit;        // table form: what the first column of this task's rows holds
};
struct DecodeBatch {
    DecodeTask tasks[kDecodeBatchMax];
    int n_tasks;
    int pad;
};
long long decode_tiles(size_t n);
size_t decode_batch_scratch_bytes(long long total_tiles, int n_tasks);
// totals_host_pinned: 2 * n_tasks values (runs begun, runs ended -- equal) after the synchronisation
int launch_decode_runs_batch(const DecodeBatch &batch, long long total_tiles, void *scratch_dev,
                             unsigned long long *totals_host_pinned, hipStream_t stream);
// the same as ONE table of (unit, begin, end) rows, task after task; `eager_rows` rows are copied to
// `table_host_pinned` in front of the synchronisation, together with the totals (no synchronisation of its own
// when eager_rows covers the table)
int launch_decode_runs_table(const DecodeBatch &batch, long long total_tiles, void *scratch_dev, int64_t *table_dev,
                             unsigned long long *totals_host_pinned, int64_t *table_host_pinned, size_t eager_rows,
                             hipStream_t stream);

// ---- objective.hip --------------------------------------------------------------------------
size_t objective_scratch_bytes(size_t n);
int launch_objective(const uint8_t *solution_dev, const double *scores_dev,
                     const double *switch_costs_dev, double gamma, size_t n, void *scratch_dev,
                     double *objective_host_pinned, hipStream_t stream, bool synchronize = true);

// several problems at once: tasks_dev[t].tile_begin = first tile of task t (objective_tiles(n) tiles each);
// partial_dev: 2 * total_tiles doubles; out_dev: n_tasks doubles (no copy, no synchronisation)
struct ObjectiveTask {
    const uint8_t *solution;
    const double *scores;
    const double *switch_costs;  // n-1 or nullptr
    double gamma;
    long long n;
    long long tile_begin;
};
long long objective_tiles(size_t n);
int launch_objective_batch(const ObjectiveTask *tasks_dev, int n_tasks, long long total_tiles, double *partial_dev,
                           double *out_dev, hipStream_t stream);

// ---- whittaker.hip --------------------------------------------------------------------------
// factor_dev: 6 * factor_cap doubles filled by launch_whittaker_factor for a length factor_cap >= cols and
// the same penalty; scratch: at least whittaker_scratch_bytes(rows, cols) bytes; matrix and output must
// not overlap
size_t whittaker_scratch_bytes(size_t rows, size_t cols);
int launch_whittaker_factor(size_t cap, double penalty_lambda, double *factor_dev, hipStream_t stream,
                            const double *old_factor_dev = nullptr, size_t old_cap = 0);
// the same table walked by two host threads and copied up (whittaker_host.cpp): same bits, a tenth of the time; returns
// with the stream drained
int build_whittaker_factor_on_host(size_t cap, double penalty_lambda, double *factor_dev, hipStream_t stream,
                                   const double *old_factor_dev = nullptr, size_t old_cap = 0);
// one group of rows of one matrix over one SEGMENT of its loci: a workgroup of the row-parallel sweeps (whittaker.hip).
// Tiles are 64 loci, counted from locus 0.  The workgroup writes the tiles [tile_begin, tile_end); a segment that does not
// start where the sweep starts first walks `warm_tiles` tiles ahead of it (below tile_begin forward, above tile_end
// backward) from a zero state, leaves the state it reaches in `spec` and goes on from it; the state at the segment's far
// end goes to `edge`.  spec / edge: 2 x group rows chains x (last value, the one before), see whittaker.hip.
struct WhittakerRowTask {
    const double *src0, *src1;
    double *dst0, *dst1;
    long long n;
    int row0, rows;
    const double *tail;  // the three factor entries per parity that depend on the length
    long long tile_begin, tile_end;
    long long warm_tiles;
    double *spec, *edge;
    // round 5: the two elementwise passes around the sweeps ride on them.  offsets (may be null): one value per row of the
    // matrix, the sweeps' input is  src - offsets[row]  (the pilot offset of rocco/inference.py:330-331); minus (backward
    // only, may be null): the forward sweep's input matrix -- dst0 receives  (minus - offsets[row]) - baseline  instead of
    // the baseline (inference.py:335), and *bad is raised when a baseline is not finite (inference.py:207-208)
    const double *offsets, *minus;
    int *bad;
};
// one matrix of a batch for the seam check behind a sweep (whittaker.hip: whittaker_seam_kernel)
struct WhittakerSeamMatrix {
    const double *src0, *src1;  // as the sweep's tasks
    double *dst0, *dst1;
    long long n;
    int rows;
    int n_seg;                 // segments per row
    int group_rows;            // rows per workgroup (the matrix's rows dealt evenly)
    long long seg_tiles;       // tiles per segment (the last one may be shorter)
    long long task_base;       // the matrix's first task: task = task_base + group * n_seg + segment
    const double *tail;
    const double *offsets, *minus;  // as the sweep's tasks
    int *bad;
};
// several matrices of one penalty (the chromosomes of a genome) in ONE pair of launches (+ one seam check each);
// tasks_host_pinned: room for whittaker_batch_stage_bytes(...), must stay untouched until the stream has passed the copy
size_t whittaker_batch_scratch_bytes(const size_t *rows, const size_t *cols, size_t count);
size_t whittaker_batch_stage_bytes(const size_t *rows, const size_t *cols, size_t count);
int whittaker_group_rows();  // rows per workgroup of the batched sweeps
// how often a segment's warm-up had NOT reached the row's own values at the seam (each such seam was recomputed from
// the true state: results are the sequential sweep's either way); process-wide, for tests and diagnostics
long long whittaker_seam_repairs();
// what launch_crossfit_whittaker_batch would do now with these shapes and flags (nothing is launched): per matrix the
// segments per row (0: no sweep walks it) and the tiles per segment; info_out[4] = the budget in loci, the warm-up in
// tiles, the workgroups per sweep, the path (0: whittaker_sweep_kernel per row, 1: the grouped rows kernels)
int whittaker_batch_plan(const size_t *rows, const size_t *cols, size_t count, int residual, int with_offsets, int *n_seg_out,
                         long long *seg_tiles_out, long long *info_out);
// after the stream of a batch launch has been waited for; returns non-zero when a residual launch met a non-finite baseline
int whittaker_collect_repairs(const void *tasks_host_pinned);
// offsets_dev (may be null, entries may be null): per matrix, one value per row that the sweeps subtract from their input;
// residual != 0: baselines_dev[i] receives (matrix - offsets) - baseline instead of the baseline (must not be the matrix)
int launch_crossfit_whittaker_batch(const double *const *matrices_dev, const size_t *rows, const size_t *cols, size_t count,
                                    double penalty_lambda, const double *factor_dev, size_t factor_cap, double *const *baselines_dev,
                                    void *scratch_dev, void *tasks_host_pinned, hipStream_t stream,
                                    const double *const *offsets_dev = nullptr, int residual = 0);

// ---- wls.hip --------------------------------------------------------------------------------
// scratch: at least wls_scratch_bytes(K, n) bytes; synchronises the stream before returning
int wls_spatial_window(size_t n, int requested);
// up to `group_rows` (1, 2, 4 or 8: wls_rolling_group_rows) consecutive rows of one matrix for the rolling launch: `row` the
// first of them (the next n doubles further), out = window variances of the row's n - window + 1 starts (the next row's
// right behind)
struct WlsRollingTask {
    const double *row;
    long long n;
    int window;
    int rows;
    double *out;
};
constexpr int kWlsRollingGroup = 8;
int wls_rolling_group_rows(size_t total_rows);
void wls_set_rolling_group_min(int rows_per_workgroup);  // (calling thread: at least so many rows per workgroup from now on; 1, 2, 4, 8)
int launch_wls_rolling_batch(const WlsRollingTask *tasks_dev, size_t n_tasks, int group_rows, hipStream_t stream);
int wls_max_window();
size_t wls_scratch_bytes(size_t K, size_t n, int spatial_window = 0, bool own_variances = true);
int launch_score_centered_wls(const double *centered_dev, size_t K, size_t n, double lower_bound_z, double prior_df,
                              double min_effect, int use_min_effect, int spatial_window,
                              double precision_floor_ratio, double *mean_dev, double *raw_var_dev,
                              double *prior_var_dev, double *mod_var_dev, double *se_dev, double *scores_dev,
                              void *scratch_dev, double *df_out, int *window_out, hipStream_t stream, int *flag_host_pinned, const double *vas_given = nullptr,
                              int *sorted_rows_out = nullptr);

int launch_log2_selfcheck(int family, unsigned long long seed, unsigned long long first, size_t count, unsigned long long *out_dev,
                          hipStream_t stream);
// row a2 glue (wls.hip): log2(max(x, 0) + pseudocount), row medians subtracted; out may alias the input
size_t log_scale_scratch_bytes(size_t K, size_t n);
int launch_log_scale_center_rows(const double *counts_dev, size_t K, size_t n, double pseudocount, int apply_log,
                                 double *centered_out_dev, double *row_offsets_out_dev, void *scratch_dev,
                                 hipStream_t stream, int *flag_host_pinned, int center = 1);
// out = log2(max(in, 0) + pseudocount), correctly rounded; *bad_dev |= 1 if a value is not finite
int launch_log_scale(const double *in_dev, double *out_dev, size_t count, double pseudocount, int *bad_dev, hipStream_t stream);
int launch_subtract(const double *a_dev, const double *b_dev, double *out_dev, size_t count, hipStream_t stream, int *bad_dev = nullptr);

// ---- summit.hip -----------------------------------------------------------------------------
int launch_summit_offsets(const int64_t *intervals_dev, size_t n_intervals, const int64_t *centers_dev,
                          const double *effect_mean_dev, size_t n_mean,
                          const int64_t *peak_start_dev, const int64_t *peak_end_dev, size_t n_peaks,
                          int64_t *offsets_out_dev, hipStream_t stream);

// ---- assemble.hip ---------------------------------------------------------------------------
size_t union_scratch_bytes(size_t count);
int launch_union_intervals(const int64_t *values_dev, size_t count, int64_t *unique_out_dev, size_t *n_unique_out,
                           int *fixed_step_out, void *scratch_dev, hipStream_t stream);
size_t scatter_scratch_bytes(size_t K, size_t m);
int launch_scatter_tracks(const int64_t *common_dev, size_t m, const int64_t *intervals_concat_dev,
                          const double *vals_concat_dev, const size_t *offsets_host, size_t K, int out_dtype,
                          void *matrix_out_dev, void *scratch_dev, hipStream_t stream);

// ---- npsum.hip ------------------------------------------------------------------------------
size_t npsum_scratch_bytes(size_t n);
int launch_numpy_sums(const double *x_dev, size_t n, const int *modes, int n_modes, double center, double scale,
                      double threshold, void *scratch_dev, double *sums_out_host, hipStream_t stream);
int launch_multiply(const double *a_dev, const double *b_dev, double *out_dev, size_t count, hipStream_t stream);
int launch_subtract_positive_row(const double *matrix_dev, const double *row_dev, size_t K, size_t n, double *out_dev,
                                 hipStream_t stream);

int launch_bigwig_dense_fill(const int64_t *starts_dev, const int64_t *ends_dev, const double *vals_dev, size_t count,
                             double const_scale, int round_digits, double *full_out_dev, size_t capacity,
                             int64_t *first_start_out, int64_t *step_out, size_t *n_full_out, int *flags_out,
                             void *scratch_dev, hipStream_t stream);

// ---- budget_stats.hip ----------------------------------------------------------------------
struct SortedProbe {
    long long ranks[8];
    double thresholds[8];
    double shift;  // thresholds are compared with (x - shift)
    int n_ranks, n_thresholds;
};
size_t sort_f64_scratch_bytes(size_t n);
int launch_sort_f64(const double *x_dev, size_t n, double *sorted_out_dev, void *scratch_dev, hipStream_t stream);
// values_out_dev: n_ranks doubles; counts_out_dev: 2 * n_thresholds (count of (x - shift) <= t, then < t)
int launch_sorted_probe(const double *sorted_dev, size_t n, const SortedProbe &probe, double *values_out_dev,
                        long long *counts_out_dev, hipStream_t stream);
size_t autocov_scratch_bytes(size_t n, int max_lag);
// sums_out_dev[k] = sum_i (x_i - mean)(x_{i+k} - mean), k = 0..max_lag (<= 1023), in a fixed order
int launch_autocov(const double *x_dev, size_t n, double mean, int max_lag, double *sums_out_dev, void *scratch_dev,
                   hipStream_t stream);
int launch_negative_part(const double *scores_dev, double *out_dev, size_t n, hipStream_t stream);
int launch_soft_counts(const double *scores_dev, double center, double scale, double *out_dev, size_t n, hipStream_t stream);

// ---- peakscore.hip -------------------------------------------------------------------------
// scratch_dev: P * K doubles
int launch_peak_signal(const double *counts_dev, const double *lengths_dev, size_t P, size_t K, double row_scale, double pc,
                       double percentile, double *out_dev, void *scratch_dev, hipStream_t stream);
int launch_ecdf_survival(const double *stat_dev, const int *bin_dev, const double *null_values_dev, const long long *null_offsets_dev,
                         size_t P, double *out_dev, hipStream_t stream);
size_t bh_scratch_bytes(size_t m);
int launch_bh_adjust(const double *pvals_dev, size_t m, double *qvals_out_dev, void *scratch_dev, hipStream_t stream);

// ---- count.hip ------------------------------------------------------------------------------
size_t count_alignment_scratch_bytes(const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                     const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host);
// max_magnitude_out_host[k]: the largest |difference cell| or |running value| of track k (the caller's 2^24 guard)
int launch_count_alignment_records(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                   const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                   const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                   const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                                   int accumulate, float *out_dev, int64_t *max_magnitude_out_host, void *scratch_dev,
                                   hipStream_t stream);
// scratch_dev: 64 bytes
int launch_alignment_chrom_range(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev, size_t n,
                                 int64_t chrom_len, int flag_exclude, int64_t *start_out, int64_t *end_out, void *scratch_dev,
                                 hipStream_t stream);
int launch_alignment_count_tail(const float *counts_dev, size_t n, double norm_scale, int scale_by_step, double step,
                                double const_scale, int round_digits, double *vals_out_dev, int64_t *first_out,
                                int64_t *last_out, void *scratch_dev, hipStream_t stream);
// K tracks in one launch; range_out_host: 2 K values
size_t chrom_range_batch_scratch_bytes(size_t K);
int launch_alignment_chrom_range_batch(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev,
                                       const int64_t *rec_offsets_host, size_t K, int64_t chrom_len, int flag_exclude,
                                       int64_t *range_out_host, void *scratch_dev, hipStream_t stream);
// the counting and, behind it, every track's positive support; 0: a track's region or offset is invalid
size_t track_supports_scratch_bytes(const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                                    const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host);
int launch_track_supports(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev, const uint16_t *flag_dev,
                          const uint8_t *mapq_dev, const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t K,
                          const rocco_hip_count_options *options_host, const rocco_hip_count_region *regions_host,
                          const int64_t *out_offsets_host, const double *norm_scale_host, int scale_by_step, double step,
                          double const_scale, float *out_dev, int64_t *max_magnitude_out_host, int64_t *support_out_host,
                          void *scratch_dev, hipStream_t stream);

// ---- track_matrix.hip -------------------------------------------------------------------------
// out_dtype: 0 float64, 1 float32; queues one launch and waits for nothing
int launch_track_matrix_fill(const float *counts_dev, size_t counts_len, const int64_t *rows_dev, size_t n_rows, const int64_t *segs_dev,
                             size_t n_segs, size_t m, int scale_by_step, double step, double const_scale, int round_digits,
                             int out_dtype, void *matrix_out_dev, hipStream_t stream);

// ---- interval_count.hip -----------------------------------------------------------------------
// 0: the shape is out of range
size_t count_intervals_scratch_bytes(const int64_t *rec_offsets_host, size_t F, size_t C, size_t P);
// out_dev: int32 [P][F]; track_facts_out_host: 2 * F * C ints (largest span, pos does not ascend)
int launch_count_alignment_intervals(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                     const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                     const int64_t *rec_offsets_host, size_t F, size_t C, const rocco_hip_count_options *options_host,
                                     const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev, size_t P,
                                     int32_t *out_dev, int32_t *track_facts_out_host, void *scratch_dev, hipStream_t stream);

// the same for S option sets, with the counts placed at out_dev[row[p] * out_stride + col0 + f]; 0: the shape is out of range
size_t count_intervals_sets_scratch_bytes(const int64_t *rec_offsets_host, size_t F, size_t C, size_t P);
int launch_count_alignment_intervals_sets(const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                                          const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                                          const int64_t *rec_offsets_host, size_t F, size_t C,
                                          const rocco_hip_count_options *options_host, size_t S, const int32_t *set_id_dev,
                                          const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev,
                                          const int64_t *row_dev, size_t P, int32_t *out_dev, size_t out_rows, size_t out_stride,
                                          size_t col0, int32_t *track_facts_out_host, void *scratch_dev, hipStream_t stream);

// ---- fragment_length.hip ----------------------------------------------------------------------
size_t record_flag_facts_scratch_bytes(size_t T);
int launch_record_flag_facts(const int32_t *pos_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t T,
                             int64_t *mapped_out_host, int32_t *unsorted_out_host, void *scratch_dev, hipStream_t stream);
// 0: the shape is out of range
size_t fragment_block_centers_scratch_bytes(const int64_t *rec_offsets_host, size_t T, const int64_t *contig_len_host, int block_size,
                                            int rolling_chunk_size);
int launch_fragment_block_centers(const int32_t *pos_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t T,
                                  const int64_t *contig_len_host, int flag_exclude, int max_iterations, int block_size,
                                  int rolling_chunk_size, int32_t *centers_out_host, int32_t *center_count_out_host,
                                  const int64_t *chunk_offsets_host, int32_t *density_out_dev, int32_t *rank_out_dev, void *scratch_dev,
                                  hipStream_t stream);
size_t strand_xcorr_scratch_bytes(size_t T, size_t n_blocks);
int launch_strand_xcorr_blocks(const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev, const int64_t *rec_offsets_host,
                               size_t T, const int32_t *block_track_host, const int64_t *block_start_host, size_t n_blocks,
                               const int32_t *min_lag_host, int flag_exclude, int block_size, int max_insert_size, int lag_step,
                               int32_t *best_lag_out_host, double *best_score_out_host, int32_t *fwd_sum_out_host,
                               int32_t *rev_sum_out_host, void *scratch_dev, hipStream_t stream);
size_t template_lengths_scratch_bytes(const int64_t *rec_offsets_host, size_t T);
int launch_template_lengths(const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mate_same_dev,
                            const int64_t *rec_offsets_host, size_t T, const int32_t *min_insert_host, int flag_exclude,
                            int max_insert_size, int32_t *lengths_tmp_dev, int32_t *lengths_out_dev, int64_t *count_out_host,
                            void *scratch_dev, hipStream_t stream);

// ---- bam_records.hip --------------------------------------------------------------------------
// 0: the shape is out of range
size_t bam_walk_scratch_bytes(size_t n_bytes, size_t segment_bytes);
int launch_bam_walk_records(const uint8_t *bytes_dev, size_t n_bytes, int64_t entry0, int n_ref, size_t segment_bytes, int guess_mode,
                            int64_t *offsets_out_dev, size_t capacity, int64_t *segment_entry_out_dev, int64_t *report_out_host,
                            void *scratch_dev, hipStream_t stream);
size_t bam_record_fields_scratch_bytes(int n_ref);
int launch_bam_record_fields(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *offsets_dev, size_t n, int n_ref, int32_t *tid_out_dev,
                             int32_t *pos_out_dev, int32_t *end_out_dev, int32_t *isize_out_dev, uint16_t *flag_out_dev,
                             uint8_t *mapq_out_dev, uint8_t *mate_same_out_dev, int32_t *qlen_out_dev, int64_t *contig_first_out_host,
                             int64_t *report_out_host, void *scratch_dev, hipStream_t stream);
size_t bam_stream_firsts_scratch_bytes(size_t K);
int launch_bam_stream_firsts(const int64_t *offsets_dev, const int32_t *tid_dev, size_t n, const int64_t *bounds_host,
                             const int32_t *expect_tid_host, size_t K, int64_t *firsts_out_host, int64_t *report_out_host, void *scratch_dev,
                             hipStream_t stream);

// ---- bgzf_inflate.hip -------------------------------------------------------------------------
// F: BgzfFraming (the blocks of a BAM file, row f8) or ZlibFraming (the data blocks of a bigWig file, row f10) of
// inflate_core.h; bgzf_inflate.hip instantiates both.  status_out_dev and produced_out_dev may be null.  The host twin (test
// support) is inflate_host<F> of inflate_core.h.
struct BgzfFraming;
struct ZlibFraming;
template <class F>
size_t inflate_scratch_bytes(size_t n_blocks);
template <class F>
int launch_inflate(const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks, uint8_t *out_dev, size_t n_out,
                   int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream);

// ---- bigwig_sections.hip ----------------------------------------------------------------------
// the inflated sections of bigWig files -> intervals (row f10); the rules and the host twin are bigwig_sections.h's.  The
// entry points of api.hip have checked every size; 0 scratch bytes: hipcub refused the shape
size_t bigwig_sections_scratch_bytes(size_t n_blocks, size_t n_files);
int launch_bigwig_sections_facts(const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev, const int64_t *produced_dev, size_t n_blocks,
                                 const int64_t *file_first_host, const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                 int32_t *status_out_dev, int64_t *block_first_out_dev, int64_t *file_offsets_out_host, int64_t *report_out_host,
                                 void *scratch_dev, hipStream_t stream);
int launch_bigwig_sections_emit(const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev, const int64_t *produced_dev, size_t n_blocks,
                                const int64_t *file_first_host, const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                const int64_t *block_first_dev, size_t capacity, int64_t *starts_out_dev, int64_t *ends_out_dev,
                                double *values_out_dev, void *scratch_dev, hipStream_t stream);

// ---- fragments_file.hip -----------------------------------------------------------------------
// the inflated text of fragments files -> lines, fields, bins (row f13); the rules and the host twin are fragments_rules.h's.
// The entry points of api.hip have checked every pointer and size; the launchers check what the host arrays hold
size_t fragfile_lines_scratch_bytes(size_t n_bytes, size_t entry0);
int launch_fragfile_lines(const uint8_t *bytes_dev, size_t n_bytes, size_t entry0, int64_t *starts_out_dev, size_t capacity,
                          int64_t *report_out_host, void *scratch_dev, hipStream_t stream);
size_t fragfile_fields_scratch_bytes(size_t K, size_t n_names, size_t name_bytes);
int launch_fragfile_fields(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines, int whole_file,
                           const int64_t *track_first_host, const int32_t *expect_host, size_t K, const uint8_t *names_host,
                           const int64_t *name_offsets_host, size_t n_names, const uint8_t *allow_bytes_dev, const int64_t *allow_offsets_dev,
                           size_t n_allow, const int64_t *allow_first_host, int32_t *start_out_dev, int32_t *end_out_dev, int32_t *weight_out_dev,
                           int32_t *name_out_dev, uint32_t *status_out_dev, int64_t *report_out_host, void *scratch_dev, hipStream_t stream);
size_t fragfile_count_scratch_bytes(size_t K, const rocco_hip_count_region *regions_host);
int launch_fragfile_count_batch(const int32_t *start_dev, const int32_t *end_dev, const int32_t *weight_dev, const uint32_t *status_dev,
                                const int64_t *line_offsets_host, size_t K, const rocco_hip_fragfile_options *options_host,
                                const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host, float *out_dev,
                                int64_t *max_magnitude_out_host, void *scratch_dev, hipStream_t stream);
size_t fragfile_range_scratch_bytes(size_t K);
int launch_fragfile_chrom_range_batch(const int32_t *start_dev, const int32_t *end_dev, const uint32_t *status_dev, const int64_t *line_offsets_host,
                                      const int64_t *chrom_len_host, size_t K, int64_t *range_out_host, void *scratch_dev, hipStream_t stream);
int launch_fragfile_mapped_count(const int32_t *weight_dev, const int32_t *name_dev, const uint32_t *status_dev, size_t n_lines, int count_mode,
                                 int one_read_per_bin, uint64_t *sum_out_host, void *scratch_dev, hipStream_t stream);

// ---- barcode_census.hip -----------------------------------------------------------------------
// the distinct barcodes of a fragments file and the lines of each (row f14); rule, hash, slot word and host twin are fragments_rules.h's
size_t barcode_census_insert_scratch_bytes(size_t n_lines);
int launch_barcode_census_insert(const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines, const uint8_t *allow_bytes_dev,
                                 const int64_t *allow_offsets_dev, size_t n_allow, uint64_t *slots_dev, int64_t *counts_dev, size_t capacity,
                                 uint8_t *arena_bytes_dev, size_t arena_bytes_capacity, int64_t *arena_offsets_dev, uint64_t *arena_hashes_dev,
                                 size_t arena_entries_capacity, size_t entries, size_t arena_used, uint64_t hash_mask, int64_t *report_out_host,
                                 void *scratch_dev, hipStream_t stream);
int launch_barcode_census_rehash(const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity, uint64_t *new_slots_dev,
                                 int64_t *new_counts_dev, size_t new_capacity, const uint64_t *arena_hashes_dev, size_t entries, uint64_t hash_mask,
                                 void *scratch_dev, hipStream_t stream);
int launch_barcode_census_records(const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity, size_t entries, int64_t *records_out_dev,
                                  void *scratch_dev, hipStream_t stream);

// ---- synth.hip ------------------------------------------------------------------------------
int launch_synth(void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride, uint64_t seed,
                 hipStream_t stream);

}  // namespace rocco
