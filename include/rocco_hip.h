/*
 * include/rocco_hip.h -- C ABI of librocco_hip.so, the MI355X (gfx950) implementation of ROCCO's
 * per-chromosome solve path:  K x n signal matrix -> per-locus scores -> budgeted chain solve ->
 * 0/1 vector -> merged runs (BED3 intervals).
 *
 * Convention (modelled on the reference's native backends, rocco/native/wls_backend.h:11-28 and
 * rocco/native/baseline_backend.h:12-23): plain pointers and sizes, caller-owned buffers, `int`
 * status -- 0 ok, -1 out of memory, -2 invalid argument, -3 HIP runtime error (see
 * rocco_hip_last_error).  All `*_dev` pointers are DEVICE pointers (HBM); everything else is host
 * memory.  `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 * synchronous with respect to their scalar outputs (they return after the needed readback) and
 * re-entrant across different solver handles; one handle must not be used from two host threads
 * at once.  There is no CPU fallback anywhere behind this interface.
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef ROCCO_HIP_H
#define ROCCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROCCO_HIP_OK 0
#define ROCCO_HIP_ENOMEM (-1)
#define ROCCO_HIP_EINVAL (-2)
#define ROCCO_HIP_EHIP (-3)

/* How a result was obtained (diagnostic; written to `path_out` / result.path). */
#define ROCCO_HIP_PATH_CERTIFIED 1 /* parallel delta-form kernels, certified equal to the reference */
#define ROCCO_HIP_PATH_EXACT 2     /* sequential exact emulation kernel (same IEEE op order)        */
#define ROCCO_HIP_PATH_TRIVIAL 3   /* decided without a kernel launch (e.g. n == 1)                 */
#define ROCCO_HIP_PATH_SPINE 4     /* parallel kernels + exact spine through the hazard chunks      */

typedef struct rocco_hip_solver rocco_hip_solver;

/* ABI version of this header (major * 1000 + minor). */
int rocco_hip_abi_version(void);

/* Last HIP/runtime error text for this thread ("" if none). */
const char *rocco_hip_last_error(void);

/* Create / destroy a solver handle bound to HIP device `device`.  The handle owns device scratch
 * and pinned host staging that grow on demand. */
int rocco_hip_solver_create(rocco_hip_solver **solver_out, int device);
void rocco_hip_solver_destroy(rocco_hip_solver *solver);

/* Tunables (speculation depth of the lambda search, force the exact kernel, ...).  Unknown keys
 * return ROCCO_HIP_EINVAL.  Keys: "force_exact" (0/1), "spec_depth" (1..6), "active_set" (0/1), "lean" (0/1),
 * "rolling_group_min" (1, 2, 4, 8: least rows per workgroup of the batched rolling launch -- fewer, fuller workgroups for a
 * caller that runs other work beside it; none changes a result). */
int rocco_hip_solver_set(rocco_hip_solver *solver, const char *key, long long value);

/* ---- scoring -------------------------------------------------------------------------------
 * Replaces rocco/rocco.py:243-304 `score_central_tendency_chrom`, median branch (264-265), as
 * reached from rocco/rocco.py:983-991.  `matrix_dev` is row-major [K][row_stride] (row_stride >= n,
 * in elements); dtype 0 = float64, 1 = float32 (the --low_memory matrices, readtracks.py:621).
 * K == 1 copies the row (rocco.py:254-255).  A NaN anywhere in a column gives NaN. */
int rocco_hip_score_median(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K,
                           size_t n, size_t row_stride, double *scores_dev, void *stream);

/* The same for `count` matrices of one K and element type in ONE launch (the chromosomes a rank owns: the
 * call-site loop of rocco/rocco.py:948-991 over chromosomes).  matrices_dev / n / row_strides / scores_dev are
 * host arrays of `count` entries; the results are those of `count` rocco_hip_score_median calls. */
int rocco_hip_score_median_batch(rocco_hip_solver *solver, const void *const *matrices_dev, int dtype, size_t K,
                                 const size_t *n, const size_t *row_strides, double *const *scores_dev, size_t count,
                                 void *stream);

/* ... and, reduced inside the same launch, what the budgeted solve first asks of every score array
 * (rocco/dp.py:110-111 np.min / np.max; the sum of absolute values bounds its running values):
 * stats_dev[3 i .. 3 i + 3) = min, max, sum |.| of scores_dev[i] (device memory; min / max skip NaN scores, the sum
 * carries them).  Every n[i] must be positive.  Copy them to the host and hand them to
 * rocco_hip_solve_budget_batch_stats_f64: the scores are then not read a second time. */
int rocco_hip_score_median_batch_stats(rocco_hip_solver *solver, const void *const *matrices_dev, int dtype, size_t K,
                                       const size_t *n, const size_t *row_strides, double *const *scores_dev,
                                       size_t count, double *stats_dev, void *stream);

/* The other branches of score_central_tendency_chrom (not reached from the reference's driver): the nearest-rank
 * quantile of rocco.py:267-272 -- `rank` (0-based position in the sorted column) is computed by the caller with
 * NumPy's own rule, np.quantile(np.arange(K), q, method="nearest") -- and the column mean of rocco.py:298-299
 * (rows added in order, one division).  Same matrix conventions as rocco_hip_score_median; NaN in a column gives NaN. */
int rocco_hip_score_order_statistic(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                    size_t row_stride, int rank, double *scores_dev, void *stream);
int rocco_hip_score_mean(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                         size_t row_stride, double *scores_dev, void *stream);

/* method="tmean" (rocco/rocco.py:273-297): per column the values outside [q_lo, q_hi] (the order statistics of ranks
 * rank_lo <= rank_hi: np.quantile(..., method="nearest") at tprop and 1 - tprop) are dropped and the rest averaged, summed as
 * SciPy 1.15's stats.tmean sums them (dropped values as 0.0, NumPy's pairwise order over the K entries): bit for bit. */
int rocco_hip_score_trimmed_mean(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                 size_t row_stride, int rank_lo, int rank_hi, double *scores_dev, void *stream);

/* np.power(scores, power) (rocco/rocco.py:255, 304): exact for power 2 (NumPy squares); any other exponent through the
 * device's pow -- NumPy's own pow differs between its SVML and libm builds in the last place, so no algorithm matches
 * it on every host (power 1, the driver's value, never comes here).  As in NumPy a NaN stays NaN, a negative finite value
 * under a fractional exponent gives NaN, and power 0 gives 1 for every value. */
int rocco_hip_power_f64(rocco_hip_solver *solver, const double *x_dev, double power, double *out_dev, size_t n, void *stream);

/* ---- dispersion ----------------------------------------------------------------------------
 * Replace rocco/rocco.py:307-355 `score_dispersion_chrom`, one entry per method.  Matrix conventions of
 * rocco_hip_score_median (row-major [K][row_stride], dtype 0 = float64 / 1 = float32 widened to float64, one result per
 * column); 2 <= K -- K == 1 (rocco.py:318-319, zeros) is answered by the caller.  A NaN anywhere in a column gives NaN.
 * Up to K = 100 each is ONE launch that reads the matrix once with the column in registers (only the trimmed std at
 * 80 < K < 100 reads it twice, see below); above that, rank counting and plain loops with no speed claim.  Every result is bit for bit that of
 * NumPy 2.2 / SciPy 1.15 on the same column.
 *
 * method="mad" (rocco.py:324-325, stats.median_abs_deviation(m, axis=0)): np.median of |column - np.median(column)|;
 * no sum is formed (the mean of the two middle values for even K). */
int rocco_hip_score_mad(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                        double *scores_dev, void *stream);

/* method="iqr" (rocco.py:326-327, stats.iqr(m, rng=rng, axis=0)): the upper percentile minus the lower one, each by
 * np.percentile's linear rule.  The caller turns a percentile q into (index, g) with NumPy's own arithmetic:
 * vi = (K - 1) * np.true_divide(q, 100), index = floor(vi), g = vi - index (0 <= g < 1); with a = sorted[index],
 * b = sorted[min(index + 1, K - 1)] and d = b - a the value is a + d g for g < 0.5 and b - d (1 - g) otherwise.
 * (index_lo, g_lo) belongs to the smaller percentile (SciPy sorts `rng`).  No sum is formed. */
int rocco_hip_score_percentile_range(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                     size_t row_stride, int index_lo, double g_lo, int index_hi, double g_hi,
                                     double *scores_dev, void *stream);

/* method="std" (rocco.py:328-329, np.std(m, axis=0)): sum / K, the squared deviations summed and divided by K, sqrt.
 * Summation order, both sums alike: pairwise_order == 0 adds the rows one after the other, as NumPy reduces axis 0 of a
 * matrix with n > 1; pairwise_order != 0 adds the K entries of each column in NumPy's pairwise order (see
 * rocco_hip_score_trimmed_mean), as NumPy reduces the single column of a K x 1 matrix -- K <= 1024 then (ROCCO_HIP_EINVAL
 * above; see rocco_hip_score_trimmed_std).  In the pairwise order finite entries can give NaN, as in NumPy: +-1.5e308 in
 * turn over K >= 16 rows drive one of the eight accumulators to +inf and its neighbour to -inf.  Row after row they cannot. */
int rocco_hip_score_std(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                        int pairwise_order, double *scores_dev, void *stream);

/* method="tstd" (rocco.py:330-348).  DIVERGENCE: the reference hands stats.tstd the two limits as n-vectors, which SciPy
 * cannot broadcast against the K x n matrix (ValueError for every K != n; for K == n limits along the wrong axis).
 * Built here is what its own tmean branch (rocco.py:273-297) does per column: stats.tstd(column, limits=(q_lo, q_hi),
 * inclusive=(True, True)) with q_lo / q_hi the order statistics of ranks rank_lo <= rank_hi (np.quantile(...,
 * method="nearest") at tprop and 1 - tprop).  Summation order: values outside the limits count as 0.0; the mean and the
 * squared deviations are each summed in NumPy's pairwise order over the K entries in row order and divided by the
 * number kept, and the variance is multiplied by kept / (kept - 1) (NaN when at most one value is kept).  Kept
 * infinities as in SciPy, which leaves their NaN deviations out: +inf with infinities at one end, NaN at both.
 * take_root != 0: the result is the correctly rounded sqrt of that variance.  take_root == 0: the variance itself
 * (stats.tvar), for a caller that takes the root as SciPy does -- `var ** 0.5` on a NumPy scalar is the host libm's pow,
 * which is not correctly rounded (glibc 2.35: 8 of 10 000 values differ from sqrt in the last place) and not the same
 * function on every host, so no device algorithm reproduces it everywhere.
 * The sort destroys the row order the sums need: for K <= 80 and K == 100 an unpermuted copy of the column stays in
 * registers beside the sorted one (one read of the matrix); only for 80 < K < 100 the column is read a second time.
 * K <= 1024, ROCCO_HIP_EINVAL above: the pairwise order (ranges of more than 128 terms split at n/2 rounded DOWN TO A
 * MULTIPLE OF 8, so into uneven halves) is written out to four levels (rocco_amd/csrc/pairwise_sum.h), which is NumPy's
 * order for every K up to 1928; three levels leave a block of more than 128 terms from K = 969 on.  Kept values near the
 * overflow threshold can give NaN where all are finite (see rocco_hip_score_std), as they do in SciPy. */
int rocco_hip_score_trimmed_std(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                size_t row_stride, int rank_lo, int rank_hi, int take_root, double *scores_dev, void *stream);

/* ---- chain solve at a fixed selection penalty ----------------------------------------------
 * Replaces rocco/_chain_dp.c:9-213 `solve_penalized_chain` (Python wrapper rocco/dp.py:49-86).
 * `switch_costs_dev` has n-1 entries, or is NULL to use the scalar `gamma` at every boundary
 * (what rocco/dp.py:37-46 materialises).  `solution_dev` (n bytes, 0/1) may be NULL.
 * value/count are the reference's (best_val, best_count) (rocco/_chain_dp.c:194-198); the value is
 * reproduced bit-for-bit only on the exact path, otherwise to ~1e-12 relative. */
int rocco_hip_solve_penalized_chain_f64(rocco_hip_solver *solver, const double *scores_dev,
                                        const double *switch_costs_dev, double gamma, size_t n,
                                        double selection_penalty, uint8_t *solution_dev,
                                        double *value_out, long long *count_out, int *path_out,
                                        void *stream);

/* ---- budgeted solve, one launch sequence for a batch of chromosomes -------------------------
 * Replaces rocco/dp.py:89-164 `calibrate_selection_penalty` (bracket + exactly `max_iter`
 * bisection steps on the selection penalty) for every task in the batch at once.  The bracket
 * seeds are formed as the reference does (rocco/dp.py:110-111: lower = min(s) - sum(c) - 1,
 * upper = max(s) + sum(c) + 1): min / max are computed on the device (exact), `sum_costs` must be
 * supplied by the caller as NumPy's pairwise np.sum(switch_costs) gives it, because its last bits
 * fix the midpoint sequence.
 * `max_iter` is per task and may be any count from 0 (the bracket's upper end is the answer: 2 evaluations) upwards;
 * every task of a batch may carry its own.  A NEGATIVE `max_iter` in any task makes the whole call return
 * ROCCO_HIP_EINVAL with nothing launched and `results` untouched.  (The reference's `for _ in range(max_iter)`,
 * rocco/dp.py:141, takes no step for a negative count; rocco_amd/dp.py gives its callers that behaviour by passing 0.) */
typedef struct {
    const double *scores_dev;       /* n doubles                                        */
    const double *switch_costs_dev; /* n-1 doubles or NULL (use gamma)                  */
    double gamma;
    size_t n;
    long long target_count;         /* int(floor(n * budget)), rocco/dp.py:197          */
    double sum_costs;               /* np.sum(switch_costs), rocco/dp.py:110-111        */
    int max_iter;                   /* >= 0; the reference's default is 60 (dp.py:93)   */
    uint8_t *solution_dev;          /* n bytes out                                      */
} rocco_hip_budget_task;

typedef struct {
    double selection_penalty; /* the returned `upper` (rocco/dp.py:164)                          */
    double penalized_value;   /* best_value                                                      */
    long long selected_count; /* best_count                                                      */
    int evaluations;          /* chain evaluations the reference would have made (62 normally)   */
    int path;                 /* ROCCO_HIP_PATH_*                                                */
    int passes;               /* device rounds this task took part in                            */
    int zone_iters;           /* bisection steps left at the first uncertain probe (-1: none)    */
    long long n_diff;         /* decisions left open by the final window (-1: no window)         */
    int maps;                 /* binade maps built for this task                                 */
} rocco_hip_budget_result;

int rocco_hip_solve_budget_batch_f64(rocco_hip_solver *solver, size_t n_tasks,
                                     const rocco_hip_budget_task *tasks,
                                     rocco_hip_budget_result *results, void *stream);

/* The same with the score statistics the solve starts from -- np.min(scores), np.max(scores) (rocco/dp.py:110-111)
 * and sum |scores| (bounds the running values) -- handed in by the caller: score_stats_host[3 t .. 3 t + 3) in HOST
 * memory, exactly as rocco_hip_score_median_batch_stats produced them for these very arrays (NULL: computed here,
 * as above; ignored for a batch with cost vectors).  Saves one pass over every score array and one device round. */
int rocco_hip_solve_budget_batch_stats_f64(rocco_hip_solver *solver, size_t n_tasks,
                                           const rocco_hip_budget_task *tasks, const double *score_stats_host,
                                           rocco_hip_budget_result *results, void *stream);

/* ---- delta-form evaluation (the parallel kernels behind the two solves above) ----------------
 * Count-only evaluation of the chain at several penalties in one pass over the scores, with the
 * certification statistics of DESIGN.md section 4, and the joint "window" evaluation over a
 * penalty interval.  These are what rocco_hip_solve_budget_batch_f64 drives; they are exported so
 * that the kernels can be checked bit-for-bit against their sequential definition
 * (oracle/delta_oracle.c) and so that callers can run their own searches.  They stand where the
 * reference calls rocco/_chain_dp.c once per penalty (rocco/dp.py:113-162). */
typedef struct {
    long long count;     /* selected loci under the exact-rule classes                          */
    long long uncertain; /* loci whose class is not certified                                   */
    long long effect;    /* bound on |count(reference) - count| (n + 1 if the model overflowed) */
    long long max_run;   /* longest run without a clear clamp behind a locus with tolerance      */
} rocco_hip_probe_stats;

/* `emap_dev`: per-chunk binade codes (ceil(n / 32) bytes, see rocco_hip_delta_build_map_f64) or NULL. */
int rocco_hip_delta_probe_f64(rocco_hip_solver *solver, const double *scores_dev,
                              const double *switch_costs_dev, double gamma, size_t n,
                              const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas,
                              rocco_hip_probe_stats *stats_out, void *stream);

/* Binade map at penalty lambda_ref: for every 32-locus chunk, the binade of the reference's running
 * value (rocco/_chain_dp.c:118-129 operate on prev0 / prev1 of that magnitude) and whether it keeps
 * a distance > margin from every power of two.  Writes ceil(n / 32) bytes to emap_dev. */
int rocco_hip_delta_build_map_f64(rocco_hip_solver *solver, const double *scores_dev,
                                  const double *switch_costs_dev, double gamma, size_t n,
                                  double lambda_ref, double margin, uint8_t *emap_dev, void *stream);

/* The same codes from the lean kernels the budgeted solve uses for the first map of its compacted problems (lean.hip:
 * lean_map_kernel, lean_mapcode_kernel: one tile kernel + one code kernel instead of six launches); scalar switch cost,
 * n >= 2.  Exported so that the two builders can be compared byte for byte. */
int rocco_hip_delta_build_map_lean_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                       double lambda_ref, double margin, uint8_t *emap_dev, void *stream);

typedef struct {
    long long count_lo, count_hi; /* selected loci of fill(LO) / fill(HI)                 */
    long long n_diff;             /* loci whose class differs between LO and HI           */
    int diff_adjacent;            /* every difference is one class step                   */
    int overflow;                 /* tolerance model exceeded somewhere                   */
    long long max_run;
    long long diff_locus[16];     /* first differences, ascending (-1 = unused)           */
    double diff_margin_lo[16], diff_margin_hi[16];
    long long diff_run[16];
    int diff_cls_lo[16], diff_cls_hi[16];
} rocco_hip_window_stats;

/* Writes fill(LO) (n bytes) to solution_dev. */
int rocco_hip_delta_window_f64(rocco_hip_solver *solver, const double *scores_dev,
                               const double *switch_costs_dev, double gamma, size_t n,
                               const uint8_t *emap_dev, double lambda_lo, double lambda_hi,
                               uint8_t *solution_dev, rocco_hip_window_stats *stats_out, void *stream);

/* The counts rocco_hip_delta_probe_f64 gives -- what rocco/_chain_dp.c returns as best_count at each penalty, through
 * the rounding model of oracle/delta_oracle.c -- from the lean kernel that carries several penalties per workgroup
 * (lean.hip: lean_model_kernel; what the budgeted solve runs on its compacted problems).  It certifies more
 * conservatively than the full kernels: open_out[i] != 0 says counts_out[i] is NOT certified equal to the reference's
 * (the solve repeats such a penalty with the full kernels); open_out[i] == 0 says it is.  Needs a binade map
 * (rocco_hip_delta_build_map_f64); scalar switch cost only; n >= 2. */
int rocco_hip_delta_model_lean_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                   const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas,
                                   long long *counts_out, long long *open_out, void *stream);

/* Count-only evaluation in exact arithmetic on the problem's grid q (the "bound" evaluation of DESIGN.md
 * section 4.4: no rounding model; shifted by -/+ eps it brackets what rocco/_chain_dp.c returns as
 * best_count), in `n_rounds` rounds of up to 32 penalties each (round r holds round_sizes[r] of them).  A round
 * whose penalties all lie at or above a penalty of the round before it runs on the loci that one selected
 * (the selected sets are nested in the penalty) -- the counts are the same, the
 * work is not.  lambdas_used_out: the penalties as evaluated (snapped to the grid); level_len_out[r]: loci
 * of the array round r ran on (n = the caller's).  Scalar switch cost only. */
int rocco_hip_delta_bound_rounds_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                     const double *lambdas, const int *round_sizes, int n_rounds,
                                     double *lambdas_used_out, long long *counts_out, long long *level_len_out,
                                     void *stream);

/* Exact counts (and optionally one exact solution) for up to 64 penalties through the "spine":
 * the parallel kernels record per-chunk state, then one wavefront per chromosome carries the
 * reference's running values exactly -- stepping only through the chunks where the parallel
 * recursion is not provably the reference's own.  `emap_dev` must be a map
 * built by rocco_hip_delta_build_map_f64 at (or near) these penalties.  counts_out[i] is what
 * rocco/_chain_dp.c returns as best_count for lambdas[i]; solution_dev (n bytes) receives the
 * solution of lambdas[solution_index] when solution_index >= 0. */
int rocco_hip_delta_spine_f64(rocco_hip_solver *solver, const double *scores_dev,
                              const double *switch_costs_dev, double gamma, size_t n,
                              const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas,
                              int solution_index, uint8_t *solution_dev, long long *counts_out,
                              void *stream);

/* ---- objective ------------------------------------------------------------------------------
 * Replaces rocco/dp.py:16-34 `objective_value`: -(s . z) + c . |diff z|  (fixed-order tree sum;
 * the reference uses BLAS dot, so agreement is to relative 1e-12, not bitwise). */
int rocco_hip_objective_value_f64(rocco_hip_solver *solver, const uint8_t *solution_dev,
                                  const double *scores_dev, const double *switch_costs_dev,
                                  double gamma, size_t n, double *objective_out, void *stream);

/* ---- run-length decode ------------------------------------------------------------------------
 * Replaces the per-locus Python loop + merge of rocco/rocco.py:180-190 (`chrom_solution_to_bed`)
 * and rocco/rocco.py:74-95 (`_merge_bed_records`) for contiguous fixed-step loci: maximal runs of
 * selected loci among loci 0..n-2 (the last locus is never emitted, rocco.py:180) are written as
 * half-open locus index pairs [run_begin, run_end) in ascending order; the interval in base pairs
 * is (intervals[run_begin], intervals[run_end]).  At most `capacity` runs are written;
 * *n_runs_out is the total found. */
int rocco_hip_decode_runs(rocco_hip_solver *solver, const uint8_t *solution_dev, size_t n,
                          int64_t *run_begin_dev, int64_t *run_end_dev, size_t capacity,
                          size_t *n_runs_out, void *stream);

/* The same for `count` solutions in three launches and ONE synchronisation (the chromosomes a rank owns; the loop
 * over chromosomes of rocco/rocco.py:1176-1196).  Host arrays of `count` entries; n_runs_out[i] may exceed
 * capacities[i] (then only the first capacities[i] runs were written: call again with more room). */
/* The same as ONE table: the runs of solution i, in ascending order, are rows row_offsets_out[i] .. row_offsets_out[i + 1]
 * of table_dev, each row three int64 (units[i], run_begin, run_end) -- what a rank hands to the interval gather
 * (exchange 2) or reads back to write its BED records.  count <= 48.  row_offsets_out has
 * count + 1 entries; when row_offsets_out[count] > capacity_rows only the first capacity_rows rows were written: call
 * again with more room.  table_host_out (may be NULL): receives a pointer to the table in pinned host memory owned by
 * the solver, valid until the next call on this solver (NULL when the table did not fit): the rows that exist are copied
 * there by a kernel in front of the call's one synchronisation (their number is known on the device only; `eager_rows`, the
 * size of an earlier host-sized copy, is ignored). */
int rocco_hip_decode_runs_table(rocco_hip_solver *solver, size_t count, const uint8_t *const *solutions_dev, const size_t *n,
                                const long long *units, int64_t *table_dev, size_t capacity_rows, size_t eager_rows,
                                size_t *row_offsets_out, const int64_t **table_host_out, void *stream);
int rocco_hip_decode_runs_batch(rocco_hip_solver *solver, size_t count, const uint8_t *const *solutions_dev, const size_t *n,
                                int64_t *const *run_begin_dev, int64_t *const *run_end_dev, const size_t *capacities,
                                size_t *n_runs_out, void *stream);

/* ---- row baselines ------------------------------------------------ */
/* Cross-fit Whittaker baseline of every row of a row-major rows x cols matrix.
 * Replaces rocco_crossfit_whittaker_baseline_matrix_f64 (rocco/native/baseline_backend.h:12-23,
 * baseline_backend.c:305-334) as called through rocco/_baseline.c:16-104 from rocco/inference.py:185-209,
 * on device buffers: same arguments, same results bit for bit, cols < 25 -> zeros.  matrix_dev and
 * baseline_out_dev must not overlap.  Returns 0, ROCCO_HIP_ENOMEM (the reference's -1) or EINVAL / EHIP. */
int rocco_hip_crossfit_whittaker_baseline_matrix_f64(rocco_hip_solver *solver, const double *matrix_dev,
                                                     size_t rows, size_t cols, double penalty_lambda,
                                                     double *baseline_out_dev, void *stream);
/* The same for `count` matrices of ONE penalty -- the chromosomes of a genome -- in one pair of launches: every group of
 * 8 rows of every matrix is a workgroup, and the pair lasts as long as the longest row (the loop over chromosomes of
 * rocco/rocco.py:948-1018 around the call of rocco/inference.py:198-206).  Host arrays of `count` entries. */
int rocco_hip_crossfit_whittaker_baseline_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                    const size_t *rows, const size_t *cols, double penalty_lambda,
                                                    double *const *baselines_dev, void *stream);
/* The batch form with the two elementwise statements around the fit folded into its sweeps (rocco/inference.py:330-338:
 * `global_centered = log_matrix - offsets; local = baseline(global_centered); centered = global_centered - local`):
 * centered_out_dev[i] = (matrices_dev[i] - row_offsets_dev[i][row]) - baseline of (matrices_dev[i] - row_offsets_dev[i][row]),
 * every operation rounded as the separate statements round it.  row_offsets_dev (may be NULL, entries may be NULL): K_i doubles per
 * matrix.  centered_out_dev[i] must not be matrices_dev[i].  ROCCO_HIP_EINVAL ("Local baseline fit produced non-finite values",
 * inference.py:207-208) when a baseline is not finite. */
int rocco_hip_crossfit_whittaker_residual_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                    const double *const *row_offsets_dev, const size_t *rows, const size_t *cols,
                                                    double penalty_lambda, double *const *centered_out_dev, void *stream);

/* The same with the sweeps' scratch (the forward sweep's two parities: twice the matrices' bytes, + records) in a block of
 * the caller's -- a framework that pools device memory keeps one pool that way instead of two that cannot see each other's reserves
 * (round 5: the composed driver's budget null wanted the ~100 GB a K = 100 genome's sweeps had left idle in the solver).
 * scratch_dev: at least rocco_hip_whittaker_batch_scratch_bytes(count, rows, cols) bytes, aligned to 256. */
size_t rocco_hip_whittaker_batch_scratch_bytes(size_t count, const size_t *rows, const size_t *cols);
int rocco_hip_crossfit_whittaker_residual_batch_scratch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                            const double *const *row_offsets_dev, const size_t *rows,
                                                            const size_t *cols, double penalty_lambda, double *const *centered_out_dev,
                                                            void *scratch_dev, size_t scratch_bytes, void *stream);

/* ---- centred-WLS locus scores ------------------------------------
 * Replaces rocco_score_centered_wls_f64 (rocco/native/wls_backend.h:11-28, wls_backend.c:744-947) as
 * called through rocco/_wls.c from rocco/inference.py:231-299 (`_score_centered_wls_matrix`), on device
 * buffers: centered_dev is the row-major K x n matrix of baseline-subtracted tracks; the six outputs are
 * n doubles each; *df_out / *window_out (host, may be NULL) receive the degrees of freedom and the
 * spatial window used.  Same arguments and, on finite input, the same results bit for bit.  Differences:
 * non-finite values are rejected with EINVAL (the reference drops such pairs from the trend fit).  Any spatial
 * window is taken (up to 63 loci the rolling sums run on LDS tiles, above that straight from memory; the
 * reference's caller always passes 31).
 * Returns 0, ROCCO_HIP_ENOMEM (the reference's -1), EINVAL (its -2) or EHIP. */
int rocco_hip_score_centered_wls_f64(rocco_hip_solver *solver, const double *centered_dev, size_t K, size_t n,
                                     double lower_bound_z, double prior_df, double min_effect, int use_min_effect,
                                     int spatial_window, double precision_floor_ratio, double *mean_dev,
                                     double *raw_var_dev, double *prior_var_dev, double *mod_var_dev, double *se_dev,
                                     double *scores_dev, double *df_out, int *window_out, void *stream);
/* The first step of the scoring above -- every row's rolling AR(1) innovation variances (wls_backend.c:610-742) -- for the
 * rows of `count` matrices in ONE launch (the chromosomes of a genome; one workgroup per row, two per compute unit):
 * variances_dev[i] receives K[i] x (n[i] - window_i + 1) doubles, window_i = the spatial window the scoring resolves for
 * n[i] (at most 63 here).  rocco_hip_score_centered_wls_given_variances_f64 is the scoring with that step already done
 * (variances_dev == NULL: the plain call). */
int rocco_hip_wls_rolling_variances_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *centered_dev,
                                              const size_t *K, const size_t *n, int spatial_window, double *const *variances_dev,
                                              void *stream);
int rocco_hip_score_centered_wls_given_variances_f64(rocco_hip_solver *solver, const double *centered_dev, size_t K, size_t n,
                                                     double lower_bound_z, double prior_df, double min_effect, int use_min_effect,
                                                     int spatial_window, double precision_floor_ratio, const double *variances_dev,
                                                     double *mean_dev, double *raw_var_dev, double *prior_var_dev, double *mod_var_dev,
                                                     double *se_dev, double *scores_dev, double *df_out, int *window_out, void *stream);

/* Diagnostic of the log scale above: the device's log2 is a two-stage evaluation (a fast double-double stage accepted when its
 * result survives its error bound on either side, else a full one with error ~2^-100); this runs `count` inputs of a family
 * (0: any positive finite bit pattern, 1: next to 1, 2: the integers first .. first + count - 1, 3: mantissas next to the
 * table's cell boundaries in random binades, 4: uniform in [0.5, 4)) through both and through the full stage alone and
 * returns in *mismatches_out how many results differ (0 expected). */
int rocco_hip_log2_selfcheck(rocco_hip_solver *solver, int family, unsigned long long seed, unsigned long long first, size_t count,
                             unsigned long long *mismatches_out, void *stream);

/* How many rows of this solver's last centred-WLS call fitted their variance trend on the sorted path (two radix sorts of the
 * row's pairs: rows shorter than 4096 loci, rows with a run of equal |value| across a bin boundary, rows with more than 8192
 * values in one cell of the rank finder) instead of the sort-free one.  Diagnostic: the results are the same either way. */
int rocco_hip_wls_sorted_rows(const rocco_hip_solver *solver);

/* ---- count-path glue of score_loci_wls ---------------------------------
 * Replaces the NumPy statements of rocco/inference.py:40-47 (`_log_scale_wls_matrix`) and 330-331 (pilot
 * offset): centered_out[k][i] = log2(max(counts[k][i], 0) + pseudocount) - median_i(log2(...)[k][:]).
 * The row medians are exact order statistics (np.median: mean of the two middle values for even n); the
 * logarithm is CORRECTLY ROUNDED (log2_cr.h; see rocco_hip_log_scale_f64 below).  NumPy's own log2 is an SVML
 * routine or libm's, neither correctly rounded: it is one ulp off on ~0.03 % of integer counts, and what that does
 * downstream is measured in tests/test_gpu_score_loci_wls.py and stated in INTEGRATION.md section 5.  centered_out_dev
 * may alias counts_dev; row_offsets_out_dev (K doubles, may be NULL) receives the medians.  apply_log2 == 0
 * takes the matrix as already log-scaled (only the pilot offset is removed; bit-exact).  Non-finite
 * input -> EINVAL (the reference raises ValueError). */
/* out = log2(max(values, 0) + pseudocount) elementwise (`_log_scale_wls_matrix`, rocco/inference.py:40-47), CORRECTLY
 * ROUNDED.  The reference calls np.log2, which is an AVX-512 SVML routine or libm's log2 depending on the host; neither
 * is correctly rounded (in this image ~0.03 % of integer counts are one ulp off) and they differ from each other, so
 * the correctly rounded value is the host-independent target.  ROCCO_HIP_EINVAL for a non-finite value. */
int rocco_hip_log_scale_f64(rocco_hip_solver *solver, const double *values_dev, size_t count, double pseudocount, double *out_dev,
                            void *stream);

int rocco_hip_log_scale_center_rows_f64(rocco_hip_solver *solver, const double *counts_dev, size_t K, size_t n,
                                        double pseudocount, int apply_log2, double *centered_out_dev,
                                        double *row_offsets_out_dev, void *stream);

/* The same log scale and the same row medians WITHOUT subtracting them: log_out_dev = log2(max(counts, 0) + pseudocount)
 * (may alias counts_dev), row_offsets_out_dev (K doubles, required) = the medians (rocco/inference.py:330).  For callers whose next
 * pass subtracts the offsets on its way (rocco_hip_crossfit_whittaker_residual_batch_f64): one pass over the matrix less. */
int rocco_hip_log_scale_row_offsets_f64(rocco_hip_solver *solver, const double *counts_dev, size_t K, size_t n,
                                        double pseudocount, int apply_log2, double *log_out_dev, double *row_offsets_out_dev,
                                        void *stream);

/* out = a - b, element by element (rocco/inference.py:335 `centered = global_centered - local_baselines`);
 * out_dev may alias a_dev or b_dev. */
int rocco_hip_subtract_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                           size_t count, void *stream);
/* out = a - b with the reference's check on b folded in (rocco/inference.py:207-208, "Local baseline fit produced non-finite
 * values"): ROCCO_HIP_EINVAL when b holds a non-finite value.  Synchronises the stream. */
int rocco_hip_subtract_finite_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                                  size_t count, void *stream);

/* ---- narrowPeak summit offsets ---------------------------------------
 * Replaces the per-peak NumPy statements of rocco/rocco.py:838-872 (`_write_narrowpeak_summit_offsets`) over the
 * summit track of rocco/rocco.py:809-835 (`_cpy_narrowpeak_summit_track`), for the peaks of one chromosome:
 * intervals_dev = the chromosome's locus starts (ascending, n_intervals of them), effect_mean_dev = the WLS mean
 * per locus (n_mean doubles, rounded to float32 inside as the reference stores it), peaks as half-open base-pair
 * intervals.  offsets_out[p] = clip(centre of the first locus with the largest non-NaN mean among the loci
 * starting in [start, end) - start, 0, end - start - 1), or -1 when the peak is empty, holds no locus or no
 * finite value.  centers_dev == NULL: the centre of locus i is (intervals[i] + intervals[i+1]) // 2 and the last
 * entry of intervals only closes the last locus (rocco.py:816-822); otherwise intervals_dev / centers_dev are the
 * `starts` / `centers` arrays of a stored summit track (rocco.py:855-857), n_intervals each.  Exact (integer /
 * compare work). */
int rocco_hip_narrowpeak_summit_offsets(rocco_hip_solver *solver, const int64_t *intervals_dev, size_t n_intervals,
                                        const int64_t *centers_dev, const double *effect_mean_dev, size_t n_mean, const int64_t *peak_start_dev,
                                        const int64_t *peak_end_dev, size_t n_peaks, int64_t *offsets_out_dev,
                                        void *stream);

/* ---- signal matrix assembly --------------------------------------------
 * The NumPy statements at the end of generate_chrom_matrix (rocco/readtracks.py:614-633) on device buffers.
 * rocco_hip_union_intervals: unique_out = np.sort(np.unique(values)) (capacity `count`), *n_unique_out = its
 * length, *fixed_step_out (may be NULL) = 1 iff np.unique(np.diff(unique_out)).size <= 1 (the bigWig check,
 * readtracks.py:615-620).
 * rocco_hip_scatter_tracks: matrix[k, np.searchsorted(common, intervals_k)] = vals_k on a zero matrix (K x m,
 * row-major, out_dtype 0 = float64, 1 = float32 as with low_memory); track k owns the entries
 * offsets_host[k] .. offsets_host[k+1] of the concatenated interval / value arrays; repeated loci inside a
 * track keep the last value, as NumPy's fancy-index assignment does.  Exact. */
int rocco_hip_union_intervals(rocco_hip_solver *solver, const int64_t *values_dev, size_t count,
                              int64_t *unique_out_dev, size_t *n_unique_out, int *fixed_step_out, void *stream);
int rocco_hip_scatter_tracks(rocco_hip_solver *solver, const int64_t *common_dev, size_t m,
                             const int64_t *intervals_concat_dev, const double *vals_concat_dev,
                             const size_t *offsets_host, size_t K, int out_dtype, void *matrix_out_dev, void *stream);

/* ---- the K x n part of the wild-bootstrap budget null -------------------
 * The random multipliers stay with NumPy on the host (rocco/inference.py:540-571 draws them from
 * np.random.default_rng streams); what moves to the device is what the reference does with them per draw
 * (rocco/inference.py:628-685 `_compute_budget_null_draw`): the K x n product, the WLS rescoring
 * (rocco_hip_score_centered_wls_f64) and the four means -- and the residual template they start from (688-722).
 * rocco_hip_numpy_sum_f64: np.sum of a contiguous float64 vector in NumPy's own order (8192-element buffer chunks,
 *   pairwise summation inside a chunk, running total over the chunks), bit for bit.
 * rocco_hip_budget_null_draw_stats_f64: stats_out[0..4) = np.mean(pos), np.mean(pos / null_soft_scale),
 *   np.mean(pos > 0), np.mean(scores > null_threshold) with pos = np.clip(scores - null_center, 0, None)
 *   (inference.py:676-684), summed in NumPy's order.
 * rocco_hip_multiply_f64: out = a * b elementwise (inference.py:665).
 * rocco_hip_subtract_positive_row_f64: out[k][i] = matrix[k][i] - max(row[i], 0) (inference.py:717-721). */
int rocco_hip_numpy_sum_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double *sum_out, void *stream);
int rocco_hip_budget_null_draw_stats_f64(rocco_hip_solver *solver, const double *scores_dev, size_t n,
                                         double null_center, double null_soft_scale, double null_threshold,
                                         double *stats_out, void *stream);
int rocco_hip_multiply_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                           size_t count, void *stream);
int rocco_hip_subtract_positive_row_f64(rocco_hip_solver *solver, const double *matrix_dev, const double *row_dev,
                                        size_t K, size_t n, double *out_dev, void *stream);

/* ---- sizing a solver's buffers ahead of a count-path batch ------------------------------------------------------
 * The count-path entries grow the solver's scratch on demand (hipMalloc + hipFree: device-wide synchronisations).  A
 * caller that runs several solver handles side by side on streams of their own (rocco_amd.inference.score_loci_wls_batch_device)
 * sizes each handle for the matrices it will see BEFORE the threads start: rows[i] x cols[i], i < count; penalty_lambda > 0
 * also builds (or extends) the device's Whittaker factor for the longest row.  rocco_hip_buffer_growths(): how many times
 * any solver buffer of the process has grown so far (diagnostic). */
int rocco_hip_count_path_reserve(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols,
                                 double penalty_lambda, void *stream);
/* sweeps_scratch_is_the_callers != 0: the baseline sweeps will get their scratch from the caller
 * (rocco_hip_crossfit_whittaker_residual_batch_scratch_f64), nothing is reserved for them */
int rocco_hip_count_path_reserve_ex(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols,
                                    double penalty_lambda, int sweeps_scratch_is_the_callers, void *stream);
long long rocco_hip_buffer_growths(void);
/* Diagnostic, process-wide since load: the batched baseline sweeps cut long rows into segments whose workgroups start from
 * a warm-up (csrc/whittaker.hip); a seam whose warm-up had not reached the row's own values is recomputed from the true
 * state -- the results are the sequential sweep's (rocco/native/baseline_backend.c:142-172) either way.  How many seams
 * (row, parity, sweep) were recomputed so far.  ROCCO_HIP_WHITTAKER_SEGMENT_LOCI / ROCCO_HIP_WHITTAKER_WARM_LOCI (read
 * per call) set the segment length (0: rows are never cut) and the warm-up. */
long long rocco_hip_whittaker_seam_repairs(void);
/* Diagnostic: what the batched baseline entries (rocco_hip_crossfit_whittaker_baseline_batch_f64, ..._residual_batch_f64)
 * would do NOW with matrices of rows[i] x cols[i], at the environment in force at the time of the call -- computed by
 * the launcher's own steps (csrc/whittaker.hip: launch_crossfit_whittaker_batch), nothing is launched and no result
 * changes.  residual: 0 for the baseline entry, 1 for the residual ones; with_offsets: non-zero when the call passes an
 * array of row offsets (the residual entries always do).  n_seg_out[i]: the segments a row of matrix i is cut into
 * (1: rows stay whole; 0: no sweep walks the matrix -- no rows, or fewer than 25 loci, baseline_backend.c:265-272);
 * seg_tiles_out[i]: 64-locus tiles per segment (the last segment may be shorter).  info_out[0]: the loci a workgroup may
 * walk (0 when ROCCO_HIP_WHITTAKER_SEGMENT_LOCI fixes the segment length); [1]: the warm-up in tiles; [2]: workgroups per
 * sweep; [3]: the path -- 0: the lone matrix of whole rows, one workgroup per row (whittaker_sweep_kernel), 1: the grouped
 * rows kernels with their seam checks.  With the default warm-up a row is first cut at 2 x warm-up + 1 tile. */
int rocco_hip_whittaker_batch_plan(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols, int residual,
                                   int with_offsets, int *n_seg_out, long long *seg_tiles_out, long long *info_out);
/* device memory the solver's scratch buffers hold now (they are kept between calls) */
long long rocco_hip_solver_device_bytes(const rocco_hip_solver *solver);
/* Diagnostic, process-wide since load: how the last bisection steps of the calibrations (rocco/dp.py:141-162) were
 * sequenced -- out[0] chains of rounding-model rounds queued by the device-side director (csrc/model_chain.h), out[1]
 * certified counts the host took over from them, out[2] counts its replay of the reference's steps was answered from
 * them without device work, out[3] counts it asked for that the chain had not evaluated (answered by regular rounds). */
void rocco_hip_model_chain_counters(long long out[4]);
/* ... and how their last step -- the window that certifies and writes the solution of the final penalty (rocco/dp.py:164, the
 * solve at `upper`) -- was served: out[0] solutions a chain wrote itself at the penalty its bisection ended at
 * (lean_write_solutions_kernel from the class words of that penalty's certified evaluation), out[1] final windows answered
 * from them without device work. */
void rocco_hip_model_chain_written_counters(long long out[2]);

/* ---- the multipliers of the bootstrap draws on the device (missing item 2) ---------------------
 * Replaces rocco/inference.py:546-575 `_generate_dependent_wild_weights` (called per row and draw at 654-664 and per
 * draw at 1206-1213): NumPy's `Generator.standard_normal` over PCG64, SciPy's `fftconvolve(..., "valid")` with the
 * Bartlett taps (inference.py:534-543), centring and scaling to unit variance.
 * rocco_hip_pcg64_standard_normal_f64: `count` values of `np.random.Generator(PCG64).standard_normal` continuing from
 *   the generator state (state, inc: the two 128-bit integers of `bit_generator.state["state"]`, high and low halves);
 *   *raw_draws_out = the 64-bit draws they consumed (`bit_generator.advance(raw_draws)` puts the host's generator
 *   where NumPy's would be).  NumPy's values bit for bit except that tail values (|x| > 3.654; 2.6e-4 of them) may
 *   differ in the last place (NumPy calls the host libm's log1p); positions in the stream never differ.
 * rocco_hip_bartlett_multipliers_f64: innovations_dev = rows x (n + n_taps - 1) row-major; weights_dev = rows x n:
 *   every row's "valid" convolution with the taps (direct sum in a fixed order -- SciPy's FFT result to ~1e-16 of the
 *   scale, not bit for bit), minus its mean, over its standard deviation.  *degenerate_out != 0: a row's deviation is
 *   <= 1e-8 (the reference then draws signs, inference.py:565-569: left to the caller; that row is returned unscaled).
 * Opt-in (`multipliers="device"` in rocco_amd.budget): the estimates agree with the host path to ~1e-12, not bit for bit. */
int rocco_hip_pcg64_standard_normal_f64(rocco_hip_solver *solver, unsigned long long state_hi, unsigned long long state_lo,
                                        unsigned long long inc_hi, unsigned long long inc_lo, size_t count, double *values_dev,
                                        unsigned long long *raw_draws_out, void *stream);
int rocco_hip_bartlett_multipliers_f64(rocco_hip_solver *solver, const double *innovations_dev, size_t rows, size_t n,
                                       const double *taps_host, size_t n_taps, double *weights_dev, int *degenerate_out,
                                       void *stream);

/* ---- score-track budget estimate: the n-long pieces (rocco/inference.py:1151-1421, 446-501; rocco/rocco.py:751-789) ----
 * rocco_hip_sort_f64: ascending sorted copy of a float64 vector (-0.0 before +0.0).  Every np.median / MAD / median
 *   of the positive scores of the estimate is an order statistic of it.
 * rocco_hip_sorted_probe_f64: values at up to 8 ranks of a sorted vector, and for up to 8 thresholds t how many
 *   elements x have (x - shift) <= t and (x - shift) < t (binary search: x - shift is monotone in x).  The sort orders bit
 *   patterns: NaNs with the sign set come first, the other NaNs last.  They satisfy no comparison and the search skips
 *   them: a count is the index of the first element past those that satisfy it, leading NaNs included (t = -inf, "<": the
 *   number of leading NaNs; t = +inf, "<=": the index of the first trailing NaN).
 * rocco_hip_autocovariance_sums_f64: sums_out[k] = sum_i (x_i - mean)(x_{i+k} - mean), k = 0..max_lag (< n; any number of lags,
 *   1024 per pair of launches), summed in a fixed order.  (The reference takes them from an FFT: agreement to ~1e-13 relative, not bitwise.)
 * rocco_hip_negative_part_f64: out = scores - clip(scores, 0, None) (the residual template of the direct-score null).
 * rocco_hip_soft_counts_f64: out = clip(scores - center, 0, None) / scale (the series whose autocorrelation time is taken). */
int rocco_hip_sort_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double *sorted_out_dev, void *stream);
int rocco_hip_sorted_probe_f64(rocco_hip_solver *solver, const double *sorted_dev, size_t n, const long long *ranks,
                               size_t n_ranks, double *values_out, double shift, const double *thresholds,
                               size_t n_thresholds, long long *counts_le_out, long long *counts_lt_out, void *stream);
int rocco_hip_autocovariance_sums_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double mean, int max_lag,
                                      double *sums_out, void *stream);
int rocco_hip_negative_part_f64(rocco_hip_solver *solver, const double *scores_dev, double *out_dev, size_t n, void *stream);
int rocco_hip_soft_counts_f64(rocco_hip_solver *solver, const double *scores_dev, double center, double scale, double *out_dev,
                              size_t n, void *stream);

/* ---- post-hoc peak scoring: the per-peak arithmetic (rocco/scores.py:180-194, 128-141, 560-583) ----
 * rocco_hip_peak_signal_stat_f64: counts_dev is [n_peaks][n_samples] (scaled counts, row-major), lengths_dev the peak
 *   lengths; stat_out[p] = np.percentile(log2(max(counts[p] * row_scale / max(int(length), 1) + pc, pc)), percentile)
 *   (`_peak_signal_stat`; the logarithm correctly rounded, see rocco_hip_log_scale_f64; np.percentile's method "linear":
 *   virtual index (n_samples - 1) * (percentile / 100); max is np.maximum: a NaN count gives a NaN statistic, and so does
 *   an interpolation between two equal infinities, as in NumPy).
 * rocco_hip_ecdf_survival_f64: bin_dev[p] selects the sorted null values null_values_dev[null_offsets_dev[b] ..
 *   null_offsets_dev[b + 1]); pvals_out[p] = (size - searchsorted_left(null, stat[p]) + 1) / (size + 1) (`EmpiricalNull.survival`;
 *   NumPy's order: a NaN statistic lies after every number, NaN null values are sorted last).
 * rocco_hip_bh_adjust_f64: Benjamini-Hochberg adjusted p-values as scipy.stats.false_discovery_control(ps, method="bh")
 *   computes them for m > 1 (p * (m / rank), running minimum from the largest rank down, clip to [0, 1]).  The caller
 *   guarantees 0 <= p <= 1 (SciPy raises otherwise; rocco_amd.scores checks it); -0.0 counts as 0. */
int rocco_hip_peak_signal_stat_f64(rocco_hip_solver *solver, const double *counts_dev, const double *lengths_dev, size_t n_peaks,
                                   size_t n_samples, double row_scale, double pc, double percentile, double *stat_out_dev, void *stream);
int rocco_hip_ecdf_survival_f64(rocco_hip_solver *solver, const double *stat_dev, const int *bin_dev, const double *null_values_dev,
                                const long long *null_offsets_dev, size_t n_peaks, double *pvals_out_dev, void *stream);
int rocco_hip_bh_adjust_f64(rocco_hip_solver *solver, const double *pvals_dev, size_t m, double *qvals_out_dev, void *stream);

/* ---- summaries along the locus axis: score quantiles and candidate masks -----------------------------------------------
 * Replace rocco/rocco.py:358-395 `cscores_quantiles` (logged per chromosome, rocco.py:1071) and rocco/inference.py:32-37,
 * 382-443 `_robust_scale`, `benjamini_hochberg`, `_standardize_wls_z_scores`, `candidate_mask_from_wls`: each is a few
 * order statistics of an n-long vector plus one elementwise pass.
 *
 * rocco_hip_select_ranks_batch_f64: for each of `count` vectors (vectors_dev / n / centers: host arrays of `count` entries)
 *   the elements at `n_ranks` (0..16) ascending 0-based ranks -- ranks is a host array [count][n_ranks], any order, duplicates
 *   allowed, each below its n -- written to values_out_dev[count][n_ranks] (device), and to counts_out_dev[count][4]
 *   (device) the number of NaNs, of -inf, of +inf and of non-NaN values <= 0.0 (-inf included) of the vector itself in
 *   either mode.  Order: the order-preserving key of the bit pattern, -0.0 before +0.0, every NaN (either sign) above +inf:
 *   -inf.. finite.. +inf.. NaN..; a selected element comes back with its own bits, a NaN as the quiet NaN with all
 *   payload bits set.  mode 0 selects among the values, mode 1 among |x - centers[v]| formed on load (subtraction and
 *   fabs as written; a non-finite x is keyed as NaN) -- what a MAD needs, with no n-long intermediate; centers may be
 *   NULL in mode 0.  A radix select: six counting passes (14 + 5 x 10 key bits) over all vectors at once, digit
 *   histograms in LDS per vector and per still-distinct prefix, one placement launch behind each; 13 launches for up to
 *   48 vectors whatever n_ranks is (more vectors: group after group of 48), no host synchronisation -- the call returns
 *   with everything queued on `stream` -- 8 bytes read per value and pass, scratch of 16384 counters per vector and
 *   nothing in proportion to n.  Results follow from integer counts alone.  n[v] < 2^31; n[v] == 0 only with n_ranks == 0.
 * rocco_hip_bh_last_passing_rank_f64: *rank_out_dev (device) = the index i into sorted_dev (rocco_hip_sort_f64's output) of
 *   the last element with sorted[i] <= fdr * ((k + 1) / (double)m) -- product and quotient in the order of inference.py:394
 *   -- or -1; sorted[i] is the cutoff of the mask.  k is the element's 0-based rank in the reference's order, where
 *   np.argsort puts every NaN last: the sort orders bit patterns, so NaNs with the sign bit set (0.0 / 0.0 on x86-64) lead
 *   its output; the kernel finds how many do (`lead`, a bisection) and takes k = i - lead, so that k == i whenever no such
 *   NaN is present.  No NaN of either sign passes.  The predicate is not monotone in k, so every rank is looked at.
 * rocco_hip_threshold_mask_f64: mask[i] = ((isfinite(x[i]) ? x[i] / divisor : 0.0) > threshold) &&
 *   (!use_floor || x[i] > floor_value), one byte 0 / 1 per element; a true IEEE division (inference.py:423, 440-442).
 * rocco_hip_at_most_mask_f64: mask[i] = x[i] <= cutoff (false for a NaN): the BH mask, p <= sorted[last passing rank].
 * rocco_hip_divide_finite_f64: out[i] = isfinite(x[i]) ? x[i] / divisor : 0.0 (`standardized`, inference.py:419-423). */
int rocco_hip_select_ranks_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *vectors_dev, const size_t *n,
                                     size_t n_ranks, const long long *ranks, int mode, const double *centers,
                                     double *values_out_dev, long long *counts_out_dev, void *stream);
int rocco_hip_bh_last_passing_rank_f64(rocco_hip_solver *solver, const double *sorted_dev, size_t m, double fdr,
                                       long long *rank_out_dev, void *stream);
int rocco_hip_threshold_mask_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double divisor, double threshold,
                                 double floor_value, int use_floor, uint8_t *mask_out_dev, void *stream);
int rocco_hip_at_most_mask_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double cutoff, uint8_t *mask_out_dev,
                               void *stream);
int rocco_hip_divide_finite_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double divisor, double *out_dev,
                                void *stream);

/* bigWig dense fill: the NumPy statements of get_bigwig_chrom_scores after the file has been read
 * (rocco/readtracks.py:141-186) for one track's intervals in ascending order (as pyBigWig returns them).
 * *flags_out: bit 0 non-finite value (147-150), bit 1 non-positive width (153-156), bit 2 variable width (158-161),
 * bit 3 start off the fixed grid (165-168), bit 4 overlapping / duplicate / out-of-order bins (170-173); nothing is
 * written when a flag is set.  Otherwise *first_start_out, *step_out and *n_full_out describe
 * np.arange(starts[0], starts[-1] + step, step); with full_out_dev != NULL and capacity >= *n_full_out it receives
 * np.round(scatter(vals) * const_scale, round_digits) (no scaling for const_scale < 0; rounding as NumPy does it:
 * multiply by 10**d, round half to even, divide).  Call once with full_out_dev == NULL for the size.  Exact. */
int rocco_hip_bigwig_dense_fill_f64(rocco_hip_solver *solver, const int64_t *starts_dev, const int64_t *ends_dev,
                                    const double *vals_dev, size_t count, double const_scale, int round_digits,
                                    double *full_out_dev, size_t capacity, int64_t *first_start_out, int64_t *step_out,
                                    size_t *n_full_out, int *flags_out, void *stream);

/* ---- decoded alignment records -> binned coverage ------------------
 * What the reference does with a BAM record once htslib has decoded it, for records any decoder supplies as six
 * arrays in file order (the order the index iterator yields them), 16 bytes per record: pos (core.pos), end
 * (bam_endpos), isize (core.isize) as int32, flag (core.flag) as uint16, mapq (core.qual) and mate_same
 * (core.mtid == core.tid) as uint8.  The records of K tracks are concatenated; rec_offsets_host has K + 1 entries.
 * BAM decoding itself is row f8; the fragments (tabix) source with its barcode filters and the count modes other than
 * "coverage", which only that source gives a meaning, is row f13 (rocco_hip_fragfile_* below); the whole-file probes
 * (paired-end detection, read length, mapped-read count, fragment length) are row f7 below.
 *
 * rocco_hip_count_alignment_records_batch: ccounts_countRegion's alignment branch (rocco/native/ccounts_backend.c:
 *   2400-2573) for K tracks in one launch series: per record the overlap test of the index iterator on the read as it
 *   lies in the file (pos < end_of_region && max(end, pos + 1) > start_of_region; a shift or an extension never brings
 *   in a read the iterator did not yield), the flag / mapping-quality filters, the paired-end or single-end fragment,
 *   the clip to the region, and either the midpoint bin (one_read_per_bin) or +1 at index0 / -1 behind index1 with the
 *   reference's clamp and skip; then the running sum over the bins.  out_dev + out_offsets_host[k] receives n_bins
 *   float32 counts of track k (accumulate != 0: they are added to what is there, one float addition per bin, as the
 *   reference adds into its countBuffer).  Integer atomics and an int32 prefix sum: the result does not depend on
 *   scheduling and equals the reference's float arithmetic while every difference cell and every running value stays
 *   within 2^24 in magnitude; max_magnitude_out_host[k] is the largest one seen for track k and the caller refuses a
 *   result beyond 2^24 (there the reference's own result depends on record order).  With accumulate and
 *   one_read_per_bin the reference adds 1.0f at a time into the used buffer: one addition per bin equals that only while
 *   the buffer holds integers, so for such a track |buffer + count| counts towards max_magnitude_out_host[k] as well and
 *   a buffer of non-integers is the caller's to avoid.  Records per track < 2^31.
 * rocco_hip_count_alignment_shape: shape_out[0..3] = records a workgroup aggregates at a time, workgroups of one
 *   launch at most, bins per scan tile, bins of the LDS window (the sizes at which the kernels change path).
 * rocco_hip_alignment_chrom_range: ccounts_getChromRange for the alignment source (ccounts_backend.c:1666-1705):
 *   *start_out = pos of the first record in file order that flag_exclude passes among those the query over
 *   [0, chrom_len) yields; *end_out = end of the LAST such record in file order (not the maximum) among those the query
 *   over [max(chrom_len - 2000000, 0), chrom_len) yields; 0 where no record qualifies (a start without an end happens).
 * rocco_hip_alignment_count_tail_f64: rocco/readtracks.py:492-517 after the counting: vals = float64(counts) *
 *   norm_scale, / step when scale_by_step, * const_scale when const_scale >= 0 (in that order); *first_out / *last_out
 *   = first / last index with vals > 0 (-1: none); vals_out_dev = np.round(vals, round_digits) for every bin (the caller
 *   slices first .. last).  Exact. */
typedef struct rocco_hip_count_options {
    int32_t flag_include, flag_exclude, min_mapq, read_length, extend_bp, paired_end_mode, min_template_length,
        max_insert_size, shift_fwd, shift_rev, one_read_per_bin;
} rocco_hip_count_options;
typedef struct rocco_hip_count_region {
    int32_t start, end, step, n_bins; /* n_bins: the reference's countBufferLength, ((end - start - 1) / step) + 1 */
} rocco_hip_count_region;
/* the four numbers of rocco_hip_count_alignment_shape; count.hip asserts that its kernels are built to them */
#define ROCCO_COUNT_CHUNK_RECORDS 512
#define ROCCO_COUNT_MAX_GRID 512
#define ROCCO_COUNT_SCAN_TILE 2048
#define ROCCO_COUNT_WINDOW_BINS 1024
int rocco_hip_count_alignment_records_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                            const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                            const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t K,
                                            const rocco_hip_count_options *options_host,
                                            const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                                            int accumulate, float *out_dev, int64_t *max_magnitude_out_host, void *stream);
void rocco_hip_count_alignment_shape(int *shape_out);
int rocco_hip_alignment_chrom_range(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                    const uint16_t *flag_dev, size_t n, int64_t chrom_len, int flag_exclude,
                                    int64_t *start_out, int64_t *end_out, void *stream);
int rocco_hip_alignment_count_tail_f64(rocco_hip_solver *solver, const float *counts_dev, size_t n, double norm_scale,
                                       int scale_by_step, double step, double const_scale, int round_digits,
                                       double *vals_out_dev, int64_t *first_out, int64_t *last_out, void *stream);

/* ---- K files of one chromosome -> its count matrix in one device pass -------------
 * What generate_chrom_matrix does over BAM inputs once the files are decoded (rocco/readtracks.py:439-518 per file,
 * 601-633 over the files), with two waits for the device per call, whatever K is, and nothing as long as the
 * chromosome crossing the bus.
 *
 * rocco_hip_alignment_chrom_range_batch: rocco_hip_alignment_chrom_range (ccounts_getChromRange, rocco/native/
 *   ccounts_backend.c:1666-1705, as rocco/readtracks.py:439-446 calls it per file) for K tracks concatenated as the batch
 *   counter takes them (rec_offsets_host: K + 1 entries): range_out_host[2 k] = pos of track k's first record in file order
 *   that flag_exclude passes, range_out_host[2 k + 1] = end of its LAST record in file order among those reaching into
 *   the last 2 000 000 bp; 0 where there is none.  One launch, one copy of 2 K int64, one wait.
 * rocco_hip_track_supports: rocco_hip_count_alignment_records_batch (same arguments, accumulate = 0) and, queued behind it
 *   without a wait, the positive support of rocco/readtracks.py:492-512 for every track: support_out_host[2 k] / [2 k + 1] =
 *   first / last bin of track k whose SCALED value float64(count) * norm_scale_host[k], / step when scale_by_step,
 *   * const_scale when const_scale >= 0 (in that order), is > 0; -1 / -1 where none is (a zero or negative scale, an
 *   underflow: a positive count alone does not decide it).  max_magnitude_out_host as the counter's.  One wait, at the end.
 * rocco_hip_track_matrix_fill: rocco/readtracks.py:505-518 per track and 614-633 over the tracks in one launch: writes
 *   every element of the n_rows x m matrix (float64, or float32 for out_dtype = 1: np.asarray(vals, dtype=float32))
 *   exactly once.  rows_dev: int64 [n_rows][ROCCO_TRACK_MATRIX_ROW_WORDS] = offset of the row's counts in counts_dev, its
 *   bins, the grid index of its bin 0 (count_start / step), the grid indices of the first and last bin of its support,
 *   the bits of its float64 norm_scale.  segs_dev: int64 [n_segs][2] = grid index and column of the first bin of each of
 *   the disjoint, ascending segments whose bins, end to end, are the m columns (segs_dev[1] = 0).  Element (k, j): with g
 *   the grid index of column j, np.round(scaled value of bin g - origin_k, round_digits) where g lies in row k's support,
 *   else +0.0.  A bin outside [0, bins) or outside counts_len is never read, whatever the tables say.  No wait: the
 *   tables and the matrix are the caller's, ordered by the stream.
 * rocco_hip_track_matrix_shape: out[0..3] = threads of a workgroup, elements of one row a workgroup writes at a time,
 *   workgroups of one launch at most (past cap x unit elements a workgroup takes several units in turn; the supports
 *   kernel shares the cap), words of a row of rows_dev. */
#define ROCCO_TRACK_MATRIX_THREADS 256
#define ROCCO_TRACK_MATRIX_UNIT 1024
#define ROCCO_TRACK_MATRIX_MAX_GRID 2048
#define ROCCO_TRACK_MATRIX_ROW_WORDS 6
int rocco_hip_alignment_chrom_range_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                          const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t K, int64_t chrom_len,
                                          int flag_exclude, int64_t *range_out_host, void *stream);
int rocco_hip_track_supports(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                             const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                             const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                             const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                             const double *norm_scale_host, int scale_by_step, double step, double const_scale, float *out_dev,
                             int64_t *max_magnitude_out_host, int64_t *support_out_host, void *stream);
int rocco_hip_track_matrix_fill(rocco_hip_solver *solver, const float *counts_dev, size_t counts_len, const int64_t *rows_dev,
                                size_t n_rows, const int64_t *segs_dev, size_t n_segs, size_t m, int scale_by_step, double step,
                                double const_scale, int round_digits, int out_dtype, void *matrix_out_dev, void *stream);
void rocco_hip_track_matrix_shape(int *out);

/* ---- decoded alignment records -> one count per (interval, file) ------------------
 * The counting half of the reference's post-hoc scoring for records already decoded (the six arrays above).
 *
 * rocco_hip_count_alignment_intervals_batch: count_alignment_intervals (rocco/_hts_counts.c:571-836) for F files in one
 *   launch series -- per interval one ccounts_countRegion call (rocco/native/ccounts_backend.c:2400-2573) with region =
 *   [start, end), intervalSizeBP = end - start and a buffer of one float, as raw_count_matrix (rocco/scores.py:250-341)
 *   uses it; at flag_exclude = 4, min_mapq = 10, one_read_per_bin = 1 it is also the pysam count of get_ecdf
 *   (rocco/scores.py:697-713; argued from the shared index iterator and filters, not run: pysam is not a dependency).
 *   F files x C contigs are T = F * C tracks, track f * C + c, concatenated; rec_offsets_host has T + 1 entries; a track
 *   may be empty.  Every track's pos must ascend (file order of an indexed BAM).  The P intervals are device arrays
 *   (contig id in [0, C), start, end; end > start; any order, overlapping, nested or repeated); one option set for the call.
 *   out_dev is int32 [P][F], row-major: exact integer counts, independent of scheduling.  (The reference adds 1.0f into
 *   one float per interval: its result is min(count, 2^24), a clamp the caller applies where it wants floats; derived
 *   from float32 arithmetic, not recorded at that depth.)  track_facts_out_host receives 2 T ints: [2 t] the largest
 *   max(end, pos + 1) - pos of track t (the width of the candidate window, so one very long record costs time on its
 *   track, never correctness), [2 t + 1] non-zero when the track's pos does not ascend -- its counts are then undefined
 *   and the caller refuses them.  One synchronisation, at the end.  P * F < 2^31 - 1.
 * rocco_hip_count_alignment_intervals_sets: the same counting for a contig group that is
 *   resident once, with the peaks and the null regions on it counted in one launch series and the counts stored at their
 *   final places.  options_host points to S option sets, 1 <= S <= ROCCO_COUNT_INTERVALS_MAX_SETS; set_id_dev is int32 [P],
 *   the set of every interval.  row_dev is int64 [P]: the count of interval p in file f goes to
 *   out_dev[row[p] * out_stride + col0 + f], out_dev being int32 [out_rows][out_stride] (out_stride: ints per row).
 *   Exactly the addressed cells are written, zeros included; every other cell of out_dev keeps its contents.  The rows of
 *   one call must be distinct: the caller's to ensure, not tested here (two intervals of one row would race).  S outside
 *   its range, out_rows = 0 or col0 + F > out_stride is ROCCO_HIP_EINVAL before anything is queued; a set id outside
 *   [0, S) or a row outside [0, out_rows) is ROCCO_HIP_EINVAL after the call's one synchronisation (the flag comes back
 *   with the track facts): no cell of such an interval is written, the other intervals' cells are.  Everything else --
 *   tracks, intervals, counts, track_facts_out_host (2 T ints, filled in both cases) -- as the call above.
 * rocco_hip_count_intervals_shape: shape_out[0..2] = candidate records of one work unit, workgroups of the counting
 *   launch at most, wavefronts per workgroup (a wavefront takes one unit at a time, in a grid stride). */
#define ROCCO_COUNT_INTERVALS_UNIT 256
#define ROCCO_COUNT_INTERVALS_MAX_GRID 1024
#define ROCCO_COUNT_INTERVALS_WAVES_PER_GROUP 4
int rocco_hip_count_alignment_intervals_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                              const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                              const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t F, size_t C,
                                              const rocco_hip_count_options *options_host, const int32_t *contig_id_dev,
                                              const int32_t *start_dev, const int32_t *end_region_dev, size_t P, int32_t *out_dev,
                                              int32_t *track_facts_out_host, void *stream);
#define ROCCO_COUNT_INTERVALS_MAX_SETS 4
int rocco_hip_count_alignment_intervals_sets(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                             const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                             const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t F, size_t C,
                                             const rocco_hip_count_options *options_host, size_t S, const int32_t *set_id_dev,
                                             const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev,
                                             const int64_t *row_dev, size_t P, int32_t *out_dev, size_t out_rows,
                                             size_t out_stride, size_t col0, int32_t *track_facts_out_host, void *stream);
void rocco_hip_count_intervals_shape(int *shape_out);

/* ---- decoded alignment records of whole files -> the facts behind the count metadata ------
 * The record passes of the reference's whole-file probes, for records already decoded: the six arrays above (the
 * query length, a seventh, is read on the host side only).  Tracks are concatenated, rec_offsets_host has T + 1 entries, a
 * track may be empty; F files x their contigs are one launch series.  Parameters arrive clamped as
 * rocco/native/ccounts_backend.c:944-967 clamps them (max_iterations >= 1, max_insert_size >= 1, block_size >= 64,
 * rolling_chunk_size >= 1, lag_step >= 1); smaller values are ROCCO_HIP_EINVAL.  Each call synchronises once, at its end.
 *
 * rocco_hip_record_flag_facts: mapped_out_host[t] = records of track t with flag & 4 == 0 -- what hts_idx_get_stat
 *   reports as mapped for a contig, all ccounts_getMappedReadCount (ccounts_backend.c:1712-1888, the loop at 1859-1874)
 *   needs; unsorted_out_host[t] != 0 when the track's pos does not ascend.  Integer reductions.
 * rocco_hip_fragment_block_centers: ccounts_backend.c:1217-1339 per track (a contig of one file): the chunk density
 *   (records passing flag_exclude and not unmapped, counted at pos / rolling_chunk_size into ceil(contig_len / chunk)
 *   int32 cells, aggregated in an LDS window of ROCCO_FRAGMENT_DENSITY_WINDOW cells per
 *   ROCCO_FRAGMENT_DENSITY_RECORDS records), the clamped window sums (winSize = block_size / chunk, at least 1, made
 *   odd; the reference's start / end rules at both contig ends), the ranking by value descending then index ascending
 *   (a stable descending radix sort) and the greedy pick of at most min(max_iterations, numChunks) centres, which stops
 *   at the first non-positive value (host code over a downloaded prefix of the ranking, extended while it runs out).
 *   The reference holds these counts in doubles; they are integers below 2^31, so int32 cells hold the same values.
 *   centers_out_host is [T][max_iterations], center_count_out_host[t] says how many are set; a contig shorter than
 *   block_size has none (1212-1215).  Optional: density_out_dev / rank_out_dev (device, int32) receive the window sums
 *   and the ranking of track t at chunk_offsets_host[t] (T + 1 entries, the chunk counts accumulated; 0 chunks for a
 *   skipped contig).
 * rocco_hip_strand_xcorr_blocks: ccounts_backend.c:1361-1469 for n_blocks blocks, one workgroup each: block b covers
 *   [block_start_host[b], + block_size) of track block_track_host[b] (the caller applies the formula and the clamp of
 *   1344-1359).  Its records are found by bisecting pos (which must ascend: rocco_hip_record_flag_facts tells) and are
 *   pos in [start, end), end <= block end, end > pos, flag_exclude passed, not unmapped -- what the index iterator and
 *   the two containment tests leave.  Forward 5' ends at pos - start and reverse 5' ends at end - 1 - start are counted
 *   in LDS (int32); fwd_sum / rev_sum are their totals; with either below 10, or no lag in range, best_lag is -1 and
 *   best_score 0.0.  Otherwise one lane per lag = min_lag_host[track], + lag_step, ... <= min(max_insert_size,
 *   block_size - 1) runs score += ((double)fwd[i] - fwdMean) * ((double)rev[i + lag] - revMean) for i = 0 ..
 *   block_size - lag - 1 in that order, multiply and add apart, so that every score has the reference's bits; best_lag
 *   is the lag of the largest score, the smallest such lag where scores compare equal (the reference's strict >),
 *   best_score its score.  A block yields a candidate iff best_lag > 0 && best_score != 0.0.  block_size is at most
 *   ROCCO_FRAGMENT_MAX_BLOCK_SIZE (two int32 arrays of a block in one workgroup's LDS); beyond it ROCCO_HIP_EINVAL.
 * rocco_hip_template_lengths: ccounts_backend.c:1115-1144: lengths_out_dev + rec_offsets_host[t] receives, in file order,
 *   |isize| of the records of track t that pass flag_exclude, are proper pairs, not read 2, have a mapped mate on the
 *   same contig and min_insert_host[t] <= |isize| <= max_insert_size; count_out_host[t] says how many.  lengths_tmp_dev
 *   and lengths_out_dev are device arrays of as many int32 as there are records.  A predicate and a stable compaction.
 * rocco_hip_fragment_length_shape: shape_out[0..3] = the four numbers below. */
#define ROCCO_FRAGMENT_THREADS 256
#define ROCCO_FRAGMENT_DENSITY_RECORDS 2048
#define ROCCO_FRAGMENT_DENSITY_WINDOW 2048
#define ROCCO_FRAGMENT_MAX_BLOCK_SIZE 20224
int rocco_hip_record_flag_facts(rocco_hip_solver *solver, const int32_t *pos_dev, const uint16_t *flag_dev,
                                const int64_t *rec_offsets_host, size_t T, int64_t *mapped_out_host, int32_t *unsorted_out_host,
                                void *stream);
int rocco_hip_fragment_block_centers(rocco_hip_solver *solver, const int32_t *pos_dev, const uint16_t *flag_dev,
                                     const int64_t *rec_offsets_host, size_t T, const int64_t *contig_len_host, int flag_exclude,
                                     int max_iterations, int block_size, int rolling_chunk_size, int32_t *centers_out_host,
                                     int32_t *center_count_out_host, const int64_t *chunk_offsets_host, int32_t *density_out_dev,
                                     int32_t *rank_out_dev, void *stream);
int rocco_hip_strand_xcorr_blocks(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev,
                                  const int64_t *rec_offsets_host, size_t T, const int32_t *block_track_host,
                                  const int64_t *block_start_host, size_t n_blocks, const int32_t *min_lag_host, int flag_exclude,
                                  int block_size, int max_insert_size, int lag_step, int32_t *best_lag_out_host,
                                  double *best_score_out_host, int32_t *fwd_sum_out_host, int32_t *rev_sum_out_host, void *stream);
int rocco_hip_template_lengths(rocco_hip_solver *solver, const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mate_same_dev,
                               const int64_t *rec_offsets_host, size_t T, const int32_t *min_insert_host, int flag_exclude,
                               int max_insert_size, int32_t *lengths_tmp_dev, int32_t *lengths_out_dev, int64_t *count_out_host,
                               void *stream);
void rocco_hip_fragment_length_shape(int *shape_out);

/* ---- the inflated bytes of a BAM file -> record offsets -> record arrays (note (29)) ------
 * What the reference's counter has htslib do per record: bam_read1 (the framing of a record and its consistency
 * checks), bam_endpos and bam_cigar2qlen.  The BGZF blocks are inflated on the host (rocco_amd/bam.py) or by rocco_hip_bgzf_inflate, further down; bytes_dev holds
 * the inflated stream of a whole file or of a slab of it.  Every load of every kernel is bounded by n_bytes: a corrupt
 * length yields a report, never an access outside the buffer.  Each call synchronises once, at its end.
 *
 * rocco_hip_bam_walk_records: the offsets of the records of bytes_dev[0, n_bytes) in stream order, the first at entry0
 *   (0 <= entry0 <= n_bytes).  The stream is cut into segments of segment_bytes (S, a power of two in [64, 2^30]; fewer
 *   than 2^31 - 1 segments).  The guess of segment i is the lowest offset o in [iS, (i + 1)S) with o + 36 <= n_bytes from
 *   which ROCCO_BAM_GUESS_DEPTH records in a row are plausible, or none; a record at p is plausible when block_size >= 32,
 *   refID and next_refID lie in [-1, n_ref), l_read_name >= 1, l_seq >= 0 and 4 n_cigar_op + l_read_name +
 *   ceil(l_seq / 2) + l_seq <= block_size - 32; a chain that runs off the stream's end behind its first record is
 *   plausible where it ends less than ROCCO_BAM_RUNOFF_BYTES past n_bytes (a slab is cut at a BGZF block boundary).  guess_mode 0 makes every guess its segment's first byte (for tests: the repair then does all the work);
 *   guess_mode 1 is the above.  The segment of entry0 always enters at entry0, those before it have none.  All segments are
 *   walked from their guesses in parallel (to the first offset >= (i + 1)S, their exit); then the true chain is followed
 *   from entry0: a guess equal to the exit of the last confirmed segment is confirmed, any other is a wrong guess and its
 *   segment is walked again from the true entry; segments the chain jumps over are overruled to none.  Only confirmed
 *   walks contribute, so the result is the sequential walk's whatever was guessed.  A walk stops at a block_size below 32
 *   (ROCCO_BAM_ERR_BLOCK_SIZE) or where the block_size word or the record it announces ends past n_bytes
 *   (ROCCO_BAM_ERR_TRUNCATED: the place to cut a slab).
 *   offsets_out_dev: int64, room for `capacity` offsets (n_bytes / 36 + 1 always suffices; ROCCO_HIP_EINVAL, with the
 *   report filled in, where it does not).  segment_entry_out_dev: optional, int64 per segment, the confirmed entry or -1.
 *   report_out_host, ROCCO_BAM_WALK_REPORT int64: [0] records, [1] the offset behind the last complete record, [2]
 *   segments, [3] wrong guesses, [4] segments walked again, [5] why the chain stopped (0: at n_bytes exactly), [6] where
 *   (-1: nowhere).
 * rocco_hip_bam_record_fields: per record r at offsets_dev[r]: tid (refID), pos, end = pos + rlen (rlen: the M, D, N, =, X
 *   lengths of the CIGAR; 0 for a record with flag 4; 0 becomes 1: bam_endpos), isize (tlen), flag, mapq, mate_same
 *   (next_refID == refID) and qlen (l_seq, or the M, I, S, =, X lengths where l_seq <= 0 and n_cigar_op > 0:
 *   bam_cigar2qlen as rocco/native/ccounts_backend.c:812-816 uses it).  Checks: the size inequality above against the
 *   true block_size (ROCCO_BAM_ERR_SIZES), l_read_name >= 1 (_READ_NAME), refID and next_refID in [-1, n_ref) (_REF_ID),
 *   the CIGAR's query length against l_seq for a mapped record with a CIGAR and l_seq > 0 (_CIGAR_SEQ), pos >= 0 where
 *   refID >= 0 (_POSITION), end < 2^31 (_END), refID ascending with -1 last (_ORDER), an offset that frames no record
 *   inside the stream (_OFFSET), and a first CIGAR operation that soft-clips exactly l_seq bases on a placed record
 *   (_CG_TAG: the real CIGAR may sit in a CG tag, which is not decoded).  report_out_host: [0] the code of the first
 *   error in record order (the lowest code within a record; 0: none), [1] its record (-1).  contig_first_out_host,
 *   n_ref + 2 int64: [k] the first record of contig k or later for k = 0 .. n_ref (records without a contig count as
 *   n_ref), [n_ref + 1] = n; meaningful when there is no error.
 * rocco_hip_bam_stream_firsts: splits a chain that was walked over n_streams streams laid one behind the other (the spans a
 *   .bai index names, rocco_amd/bam.py: read_alignment_spans) back into its streams.  offsets_dev[n]: the ascending record
 *   offsets of the walk; tid_dev[n]: their refIDs; bounds_host[n_streams + 1]: the ascending byte bounds of the streams
 *   (0 <= bound; an empty stream repeats a bound; the last is n_bytes; ROCCO_HIP_EINVAL otherwise, or for n_streams < 1);
 *   expect_tid_host[n_streams]: the refID every record of a stream must carry.  One lane per record (a grid stride under
 *   ROCCO_BAM_MAX_GRID workgroups of ROCCO_BAM_THREADS): the bounds are bisected with an upper-bound search, so a record on a
 *   repeated bound belongs to the last stream that begins there; every load is bounded by n and n_streams.
 *   firsts_out_host[n_streams + 1]: [j] the first record at or after bound j, [n_streams] = n.  report_out_host: [0] the
 *   code of the first error in stream order (the lowest code within a stream; 0: none), [1] its stream (-1):
 *   ROCCO_BAM_ERR_SEAM, a bound with records or bytes behind it is not itself a record start (the index's begin or end lay
 *   inside a record, the chain crossed the seam mis-framed); ROCCO_BAM_ERR_SPAN_TID, a record of the stream carries another
 *   refID than expected (the index is stale or another file's).  Synchronises once, at its end.
 * rocco_hip_bam_shape: shape_out[0..2] = ROCCO_BAM_GUESS_DEPTH, ROCCO_BAM_SEGMENT_BYTES (the default S), ROCCO_BAM_THREADS. */
#define ROCCO_BAM_GUESS_DEPTH 3
#define ROCCO_BAM_SEGMENT_BYTES 16384
#define ROCCO_BAM_RUNOFF_BYTES 65536
#define ROCCO_BAM_THREADS 256
#define ROCCO_BAM_WALK_REPORT 8
#define ROCCO_BAM_ERR_BLOCK_SIZE 1
#define ROCCO_BAM_ERR_TRUNCATED 2
#define ROCCO_BAM_ERR_SIZES 3
#define ROCCO_BAM_ERR_READ_NAME 4
#define ROCCO_BAM_ERR_REF_ID 5
#define ROCCO_BAM_ERR_CIGAR_SEQ 6
#define ROCCO_BAM_ERR_POSITION 7
#define ROCCO_BAM_ERR_END 8
#define ROCCO_BAM_ERR_CG_TAG 9
#define ROCCO_BAM_ERR_ORDER 10
#define ROCCO_BAM_ERR_OFFSET 11
#define ROCCO_BAM_ERR_SEAM 12
#define ROCCO_BAM_ERR_SPAN_TID 13
int rocco_hip_bam_walk_records(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, int64_t entry0, int n_ref,
                               size_t segment_bytes, int guess_mode, int64_t *offsets_out_dev, size_t capacity,
                               int64_t *segment_entry_out_dev, int64_t *report_out_host, void *stream);
int rocco_hip_bam_record_fields(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *offsets_dev, size_t n,
                                int n_ref, int32_t *tid_out_dev, int32_t *pos_out_dev, int32_t *end_out_dev, int32_t *isize_out_dev,
                                uint16_t *flag_out_dev, uint8_t *mapq_out_dev, uint8_t *mate_same_out_dev, int32_t *qlen_out_dev,
                                int64_t *contig_first_out_host, int64_t *report_out_host, void *stream);
int rocco_hip_bam_stream_firsts(rocco_hip_solver *solver, const int64_t *offsets_dev, const int32_t *tid_dev, size_t n,
                                const int64_t *bounds_host, const int32_t *expect_tid_host, size_t n_streams, int64_t *firsts_out_host,
                                int64_t *report_out_host, void *stream);
void rocco_hip_bam_shape(int *shape_out);

/* ---- the BGZF blocks of a BAM file -> their inflated bytes (note (29)) ----------------------
 * What the reference has htslib's BGZF reader do per block: inflate its DEFLATE stream (RFC 1951), compare the length with
 * the trailer's ISIZE and the CRC32 of the bytes with the trailer's CRC32.  The block headers are walked on the host
 * (rocco_amd/bam.py: _bgzf_blocks), which states every block as one row of the block table:
 *   table_dev: int64 [n_blocks][ROCCO_BGZF_TABLE_COLUMNS], one device array, a row = { the first byte of the block's
 *   deflate data in comp_dev, one past its last, ISIZE, CRC32, the offset of its bytes in out_dev (the prefix sum of ISIZE
 *   where the blocks are to lie one behind the other) }.
 *
 * rocco_hip_bgzf_inflate: comp_dev[0, n_comp) holds the compressed bytes of a file or of a slab of it; every block is
 *   inflated by one wavefront of ROCCO_BGZF_THREADS lanes into out_dev[offset, offset + ISIZE), then its CRC32 is taken
 *   (per-lane table-driven CRCs of 64 contiguous chunks, combined as zlib's crc32_combine does).  The streams are accepted
 *   and rejected exactly as zlib 1.2.11 does for a raw stream (stored, fixed and dynamic blocks, several per BGZF block,
 *   lengths to 258, distances to 32 768, overlapping copies; block type 3, LEN != ~NLEN, HLIT > 286 or HDIST > 30, an
 *   incomplete code-length code, a repeat past the lengths or a leading 16, no code for 256, over-subscribed sets,
 *   incomplete sets other than one code of length 1 or no distance code at all, the use of a missing code, a distance
 *   beyond the bytes produced and a span that ends inside the stream are rejected; bytes behind the final block are
 *   ignored).  Every load is bounded by the row's span, every store by its ISIZE: a stream that inflates to more is
 *   followed to its end without storing, and nothing outside [offset, offset + ISIZE) is written whatever the span holds.
 *   A row is refused (ROCCO_BGZF_ERR_TABLE, nothing of it read or written) unless 0 <= first <= last <= n_comp,
 *   0 <= ISIZE <= ROCCO_BGZF_MAX_ISIZE and [offset, offset + ISIZE) lies in [0, n_out).  Rows whose ranges overlap are the
 *   caller's error.
 *   status_out_dev: optional, int32 per block: 0, ROCCO_BGZF_ERR_STREAM | reason << 8 (reason 1 ..
 *   ROCCO_BGZF_STREAM_REASONS: block type, stored length, too many symbols, code-length set, repeat, no end-of-block,
 *   literal/length set, distance set, literal/length code, distance code, distance too far back, input ends), _LENGTH (the
 *   stream is sound and inflates to another length), _CRC or _TABLE; in zlib's order: a stream error before a length
 *   error before a CRC error.  report_out_host, ROCCO_BGZF_REPORT int64: [0] the first failing block in table order or
 *   -1, [1] its status, [2] the bytes it inflates to (for _LENGTH).  The bytes of blocks that fail are unspecified inside
 *   their own range.  Synchronises once, at its end.  n_blocks = 0 is a valid call.
 * rocco_hip_bgzf_inflate_host: test support, as rocco_hip_synth_matrix is: the same rows over HOST memory (comp, table, out
 *   and status_out are host pointers), on the calling thread, from the same source as the kernels (csrc/inflate_core.h
 *   compiled for the host); no device is touched, solver may be NULL.
 * rocco_hip_bgzf_shape: shape_out[0..3] = ROCCO_BGZF_THREADS, ROCCO_BGZF_TABLE_COLUMNS, ROCCO_BGZF_MAX_ISIZE,
 *   ROCCO_BGZF_STREAM_REASONS. */
#define ROCCO_BGZF_THREADS 64
#define ROCCO_BGZF_TABLE_COLUMNS 5
#define ROCCO_BGZF_MAX_ISIZE 65536
#define ROCCO_BGZF_REPORT 4
#define ROCCO_BGZF_STREAM_REASONS 12
#define ROCCO_BGZF_ERR_STREAM 1
#define ROCCO_BGZF_ERR_LENGTH 2
#define ROCCO_BGZF_ERR_CRC 3
#define ROCCO_BGZF_ERR_TABLE 4
#define ROCCO_BGZF_MAX_GRID (1 << 20) /* workgroups of inflate_kernel<BgzfFraming> and check_kernel<BgzfFraming> at most; unit: one BGZF block (a workgroup strides over the rows i, i + grid, ...) */
int rocco_hip_bgzf_inflate(rocco_hip_solver *solver, const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks,
                           uint8_t *out_dev, size_t n_out, int32_t *status_out_dev, int64_t *report_out_host, void *stream);
int rocco_hip_bgzf_inflate_host(rocco_hip_solver *solver, const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks,
                                uint8_t *out, size_t n_out, int32_t *status_out, int64_t *report_out);
void rocco_hip_bgzf_shape(int *shape_out);

/* ---- the data blocks of a bigWig file -> their inflated bytes (note (31)) -----------------
 * What libBigWig has zlib's uncompress() do per data block when pyBigWig's intervals() calls bwGetOverlappingIntervals:
 * check the two header bytes of the zlib stream (RFC 1950), inflate its deflate data, compare the Adler-32 of the bytes with
 * the four big-endian bytes behind the stream.  The container is walked on the host (rocco_amd/bigwig.py), which states
 * every block as one row of the block table:
 *   table_dev: int64 [n_blocks][ROCCO_ZLIB_TABLE_COLUMNS], a row = { the first byte of the zlib stream in comp_dev, one past
 *   its last, the capacity of its slot (the file's uncompressBufSize), the offset of its slot in out_dev (the host's stride:
 *   the capacity rounded up to 8), framing }.  Framing 0: a zlib stream.  Framing 1: stored as it is (a file whose
 *   uncompressBufSize is 0): the span's bytes are copied and produced is the span's length.
 *
 * rocco_hip_zlib_inflate: every block is taken by one wavefront of ROCCO_BGZF_THREADS lanes (a grid stride under
 *   ROCCO_ZLIB_MAX_GRID workgroups).  The header is judged as zlib 1.2.11's inflate() does with wbits = 15: (CMF * 256 + FLG)
 *   % 31 != 0 is "incorrect header check" (reason 1), CM != 8 "unknown compression method" (2), CINFO > 7 "invalid window
 *   size" (3), FDICT set is refused (4: zlib would ask for a dictionary).  The deflate data is decoded by the decoder of
 *   rocco_hip_bgzf_inflate (the same rules, the same reasons) into out_dev[offset, offset + capacity); a second kernel takes
 *   the Adler-32 of the produced bytes (64 contiguous chunks, one per lane, combined as zlib's adler32_combine does) and
 *   compares it with the four bytes at the stream's end -- the byte behind the last bit of the final deflate block.  Fewer
 *   than four bytes there (or fewer than two for the header, or fewer than four behind FDICT) is zlib's "incomplete or
 *   truncated stream"; bytes behind the Adler-32 are ignored, as uncompress() ignores them.  Every load is bounded by the
 *   row's span, every store by its slot: a stream that inflates to more than the capacity is followed to its end without
 *   storing.  A row is refused (ROCCO_BGZF_ERR_TABLE, nothing of it read or written) unless 0 <= first <= last <= n_comp,
 *   0 <= capacity <= ROCCO_BGZF_MAX_ISIZE, [offset, offset + capacity) lies in [0, n_out) and framing is 0 or 1.
 *   status_out_dev (optional, int32 per block): 0, ROCCO_BGZF_ERR_STREAM | reason << 8, ROCCO_BGZF_ERR_LENGTH (sound, and
 *   inflates to MORE than the capacity: produced <= capacity is accepted), ROCCO_BGZF_ERR_TABLE, ROCCO_ZLIB_ERR_HEADER |
 *   reason << 8, ROCCO_ZLIB_ERR_TRUNCATED or ROCCO_ZLIB_ERR_ADLER; where several hold: header, stream, truncated, length,
 *   Adler.  produced_out_dev (optional, int64 per block): the bytes the block inflates to (0 where the header or the stream
 *   is refused).  report_out_host, ROCCO_BGZF_REPORT int64: [0] the first failing block in table order or -1, [1] its
 *   status, [2] the bytes it inflates to.  The bytes of failing blocks are unspecified inside their own slot.  Synchronises
 *   once, at its end.  n_blocks = 0 is a valid call.
 * rocco_hip_zlib_inflate_host: test support, as rocco_hip_bgzf_inflate_host is: the same rows over HOST memory on the
 *   calling thread, from the same source (csrc/inflate_core.h compiled for the host); solver may be NULL.
 * rocco_hip_zlib_shape: shape_out[0..4] = ROCCO_BGZF_THREADS, ROCCO_ZLIB_TABLE_COLUMNS, ROCCO_BGZF_MAX_ISIZE,
 *   ROCCO_ZLIB_HEADER_REASONS, ROCCO_ZLIB_MAX_GRID. */
#define ROCCO_ZLIB_TABLE_COLUMNS 5
#define ROCCO_ZLIB_HEADER_REASONS 4
#define ROCCO_ZLIB_ERR_HEADER 5
#define ROCCO_ZLIB_ERR_ADLER 6
#define ROCCO_ZLIB_ERR_TRUNCATED 7
#define ROCCO_ZLIB_MAX_GRID (1 << 16) /* workgroups of inflate_kernel<ZlibFraming> and check_kernel<ZlibFraming> at most; unit: one data block */
int rocco_hip_zlib_inflate(rocco_hip_solver *solver, const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks,
                           uint8_t *out_dev, size_t n_out, int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host,
                           void *stream);
int rocco_hip_zlib_inflate_host(rocco_hip_solver *solver, const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks,
                                uint8_t *out, size_t n_out, int32_t *status_out, int64_t *produced_out, int64_t *report_out);
void rocco_hip_zlib_shape(int *shape_out);

/* ---- the inflated data blocks of bigWig files -> their intervals (note (31)) --------------
 * What libBigWig's bwGetOverlappingIntervals(bw, chrom, 0, length) does with every data block once it is inflated
 * (bwValues.c), which is what pyBigWig's intervals(chromosome) returns.  The input is what rocco_hip_zlib_inflate left:
 *   slots[0, n_slots), the block table int64 [n_blocks][ROCCO_ZLIB_TABLE_COLUMNS] (column 2 the slot's capacity, column 3
 *   its offset in slots), produced int64 [n_blocks] (the bytes of block i are slots[offset, offset + produced[i])), and
 *   for the n_files files whose blocks lie one behind the other in the table three HOST arrays: file_first int64
 *   [n_files + 1] (file k's blocks are file_first[k] .. file_first[k + 1]; ascending from 0 to n_blocks), chrom_id and
 *   chrom_length int64 [n_files] (the chromosome's id and length in file k's chromosome tree).
 * Per block, in this order (refusals are this project's: libBigWig would read past the section or wrap):
 *   the row must fit: 0 <= capacity, 0 <= offset, offset + capacity <= n_slots, 0 <= produced <= capacity, else
 *     ROCCO_BGZF_ERR_TABLE and nothing of the block is read;
 *   produced < 24: ROCCO_BIGWIG_ERR_SHORT (no room for the header, which libBigWig reads without asking);
 *   the header `<IIIIIBBH` = chromId, chromStart, chromEnd, itemStep, itemSpan, type, reserved, itemCount; chromId other
 *     than the file's chrom_id: the block is skipped whole as libBigWig skips it (status 0, no interval, nothing else judged);
 *   type outside 1 (bedGraph), 2 (variableStep), 3 (fixedStep): ROCCO_BIGWIG_ERR_TYPE (libBigWig's switch has no default);
 *   produced < 24 + itemCount * (12, 8, 4 by type): ROCCO_BIGWIG_ERR_ITEMS (libBigWig would read past the section); more
 *     bytes than that are ignored, as libBigWig ignores them;
 *   item j: (start, end, float32) | (start, float32), end = start + itemSpan | (float32), start = chromStart + j * itemStep,
 *     end = start + itemSpan, in 64-bit arithmetic; an end beyond 2^32 - 1: ROCCO_BIGWIG_ERR_WRAP (libBigWig's uint32_t
 *     would wrap around) for the whole block;
 *   an item is kept unless end <= 0 || start >= chrom_length (bwValues.c's test against the queried range [0, length)).
 * The kept items of all blocks in block order, within a block in item order, are the output: starts int64, ends int64,
 * values float64 (the float32 as C's (double) widens it: NaN payloads and zero signs stay) -- the arguments of
 * rocco_hip_bigwig_dense_fill_f64.
 *
 * rocco_hip_bigwig_sections_facts: the first call.  status_out_dev int32 [n_status >= n_blocks]: 0 or why the block is
 *   refused; block_first_out_dev int64 [n_block_first >= n_blocks + 1]: the index of every block's first kept item (a refused
 *   block keeps none), the last cell the total; file_offsets_out_host int64 [n_files + 1]: the same for the files;
 *   report_out_host, ROCCO_BGZF_REPORT int64: [0] the first refused block in table order or -1, [1] its status, [2] the total.
 *   One wavefront of ROCCO_BIGWIG_THREADS lanes per block under a grid stride of ROCCO_BIGWIG_MAX_GRID workgroups.
 *   ROCCO_HIP_EINVAL before anything is launched where a pointer is null while its size is not 0, a size is too small or
 *   file_first does not ascend from 0 to n_blocks.  Waits for the device ONCE, at its end, and returns the error state
 *   it finds there (ROCCO_HIP_EHIP): a fault of its kernels is this call's error, not a later call's.
 * rocco_hip_bigwig_sections_emit: the second call, with the same inputs and block_first_dev as the first left it; total is
 *   report[2].  Writes starts_out_dev[0, total), ends_out_dev[0, total), values_out_dev[0, total); n_starts, n_ends and
 *   n_values are the arrays' sizes in elements: ROCCO_HIP_EINVAL before anything is launched where one is smaller than
 *   total, a pointer is null while its size is not 0, or n_block_first < n_blocks + 1.  total = 0 launches nothing.  No
 *   index at or past the least of the three sizes is written whatever block_first_dev holds.  Waits once, at its end.
 * rocco_hip_bigwig_sections_host: test support, as rocco_hip_zlib_inflate_host is: both stages over HOST memory on the
 *   calling thread from the same source (csrc/bigwig_sections.h compiled for the host); solver may be NULL.  starts_out
 *   NULL (with ends_out, values_out NULL and their sizes 0): the first stage alone.  Else the items are written where no
 *   block is refused; a total beyond a size is ROCCO_HIP_EINVAL with nothing written.
 * rocco_hip_bigwig_sections_shape: shape_out[0..2] = ROCCO_BIGWIG_THREADS, ROCCO_BIGWIG_MAX_GRID, the header's 24 bytes. */
#define ROCCO_BIGWIG_THREADS 64
#define ROCCO_BIGWIG_MAX_GRID (1 << 16) /* workgroups of sections_facts_kernel and sections_emit_kernel at most; unit: one data block */
#define ROCCO_BIGWIG_ERR_SHORT 8
#define ROCCO_BIGWIG_ERR_TYPE 9
#define ROCCO_BIGWIG_ERR_ITEMS 10
#define ROCCO_BIGWIG_ERR_WRAP 11
int rocco_hip_bigwig_sections_facts(rocco_hip_solver *solver, const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev,
                                    const int64_t *produced_dev, size_t n_blocks, const int64_t *file_first_host,
                                    const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files, int32_t *status_out_dev,
                                    size_t n_status, int64_t *block_first_out_dev, size_t n_block_first, int64_t *file_offsets_out_host,
                                    int64_t *report_out_host, void *stream);
int rocco_hip_bigwig_sections_emit(rocco_hip_solver *solver, const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev,
                                   const int64_t *produced_dev, size_t n_blocks, const int64_t *file_first_host,
                                   const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                   const int64_t *block_first_dev, size_t n_block_first, size_t total, int64_t *starts_out_dev, size_t n_starts,
                                   int64_t *ends_out_dev, size_t n_ends, double *values_out_dev, size_t n_values, void *stream);
int rocco_hip_bigwig_sections_host(rocco_hip_solver *solver, const uint8_t *slots, size_t n_slots, const int64_t *table, const int64_t *produced,
                                   size_t n_blocks, const int64_t *file_first, const int64_t *chrom_id, const int64_t *chrom_length,
                                   size_t n_files, int32_t *status_out, size_t n_status, int64_t *block_first_out, size_t n_block_first,
                                   int64_t *file_offsets_out, int64_t *starts_out, size_t n_starts, int64_t *ends_out, size_t n_ends,
                                   double *values_out, size_t n_values, int64_t *report_out);
void rocco_hip_bigwig_sections_shape(int *shape_out);

/* ---- fragments files: inflated text -> lines -> fields -> bins (note (34)) ---------------
 * The reference's third counting source, ccounts_sourceKindFragments (rocco/native/ccounts_backend.c): the BGZF-compressed,
 * tabix-indexed text of single-cell ATAC pipelines, one line "contig<TAB>start<TAB>end<TAB>barcode<TAB>count" per fragment.
 * The container (the .tbi index, the BGZF blocks) is read by rocco_amd/tabix_index.py and rocco_amd/fragments.py and
 * inflated by rocco_hip_bgzf_inflate or on the host; these entries take the inflated bytes.  The rules are written once, in
 * csrc/fragments_rules.h, for the kernels and for rocco_hip_fragfile_host.
 *
 * rocco_hip_fragfile_lines: the lines of bytes_dev[entry0 .. n_bytes).  A facts kernel counts '\n' per tile of
 *   ROCCO_FRAGFILE_TILE_BYTES bytes (a grid stride under ROCCO_FRAGFILE_LINES_MAX_GRID workgroups), hipcub's exclusive sum
 *   gives every tile its first line, an emit kernel writes the line starts: starts_out_dev[0] = entry0, one entry behind
 *   every '\n' that is not the last byte, and starts_out_dev[n_lines] = n_bytes, so that line i is [starts[i], starts[i + 1])
 *   with its terminator; an unterminated last line is a line.  report_out_host[0..3] = n_lines, the offset behind the last
 *   '\n' (entry0 where there is none: where a slab is cut), 1 where the last line is unterminated, 0.  With
 *   starts_out_dev == NULL only the report is made (call once for the size); otherwise ROCCO_HIP_EINVAL where `capacity`
 *   holds fewer than n_lines + 1 entries.  No byte at or beyond n_bytes is read.
 * rocco_hip_fragfile_fields: one lane per line (ROCCO_FRAGFILE_THREADS lines per workgroup turn, a grid stride under
 *   ROCCO_FRAGFILE_FIELDS_MAX_GRID).  The lines are those of K tracks one behind the other (track_first_host[K + 1], in
 *   lines).  Per line: start and end (columns 2 and 3 by ccounts_parseInt64Field, 359-394), weight (column 5 where it
 *   parses and is positive, else 1: 2246-2249, 2271), name (the index of column 1 among the n_names packed names:
 *   names_host[name_offsets_host[i] .. name_offsets_host[i + 1]); -1 where it is none of them) and the status word below;
 *   the barcode (column 4) is looked up by binary search in the track's own sorted allow-list, the entries
 *   [allow_first_host[k], allow_first_host[k + 1]) of allow_bytes_dev / allow_offsets_dev (n_allow + 1 offsets; an empty list
 *   allows everything, as does an empty barcode: 311-357, 2261-2269).
 *   whole_file == 0, the lines of index spans: a line that begins with '#' is a meta line (the index iterator skips it) and
 *   gets the status ROCCO_FRAGFILE_META alone; every other line must keep the dialect: at least three fields, columns 2 and
 *   3 canonical decimals ("0" or [1-9][0-9]*) below 2^31, no NUL, no '\r' but directly before '\n', column 1 equal to name
 *   expect_host[k] (-1: not checked), column 2 not below that of the track's line before it, column 5 -- where it is an
 *   optional '-' and digits -- of at most 18 digits and below 2^31.  whole_file != 0, hts_getline's lines (1770, 713): meta
 *   lines and short lines are lines; the canonical rule holds for columns 2 and 3 of every other line that has them (an
 *   empty column is one the line does not have).  The range rules hold for EVERY line, meta lines included: a column 2 or 3
 *   that parses and lies at or beyond 2^31 in magnitude, and a column 5 beyond 18 digits or 2^31, are refused wherever
 *   they stand (the outputs are int32).  n_lines < 2^32.
 *   report_out_host[0..3] = the first offending line in line order (-1: none), the lowest ROCCO_FRAGFILE_ERR_* within it, 0, 0.
 * rocco_hip_fragfile_count_batch: ccounts_countRegion's fragments branch (2212-2353) for K tracks (slices of the line
 *   arrays, line_offsets_host[K + 1]; each with its own region, mode and one_read_per_bin) in one launch series.  A line
 *   counts when both integers parsed, end > start, the last field the reference's loop scans is not empty and its barcode
 *   is allowed.  center, or one_read_per_bin in any mode: weight at the bin of (start + end) / 2 where that lies in the
 *   region; cutsite and fiveprime: weight at the bin of start and at the bin of end - 1, each tested on its own; coverage:
 *   the clip to the region, +weight at index0 and -weight behind index1 with the reference's clamp and skips, then the
 *   running sum.  Integer atomics into a positive sum P and a negative sum N per bin (64-bit cells), so the result does not
 *   depend on scheduling; coverage scans P - N and converts once to float32, the other modes write P.  The reference adds
 *   floats in file order; that equals these integers for any order while max(P, N) of every cell and every running value
 *   stay within 2^24 (every partial sum of a cell lies in [-N, P]).  max_magnitude_out_host[k] is that maximum for track k;
 *   the caller refuses a result beyond 2^24.  out_dev + out_offsets_host[k] receives the n_bins counts of track k; nothing
 *   is accumulated into what was there.
 * rocco_hip_fragfile_chrom_range_batch: ccounts_getChromRange's fragments branch (1583-1631) per track: range_out_host[2 k]
 *   = start of the first line in file order whose integers parsed and whose end > start, [2 k + 1] = end of the LAST such
 *   line in file order (not the maximum); 0 / 0 where there is none.  Only lines with start < chrom_len_host[k] count: the
 *   reference's query over [0, chromLength) yields no other (1579-1580).
 * rocco_hip_fragfile_mapped_count: the sum of ccounts_getMappedReadCount's fragments branch (1770-1835) over n_lines lines
 *   of a whole-file field pass whose names were the contigs to leave out: a line counts when name < 0, its fifth field is
 *   not empty and its barcode is allowed; it adds its weight, twice for cutsite / fiveprime without one_read_per_bin.  An
 *   integer reduction into *sum_out_host.
 * rocco_hip_fragfile_host: the line pass and the field pass over HOST memory on the calling thread, from the same
 *   header (test support; no device is touched, `solver` may be NULL).  track_first may be NULL for one track over all
 *   lines (expect[0], allow_first[0..1]); the five field outputs may all be NULL for the line pass alone.
 * rocco_hip_fragfile_shape: shape_out[0..5] = ROCCO_FRAGFILE_THREADS, ROCCO_FRAGFILE_TILE_BYTES, the lines of a workgroup
 *   turn of the field, count and range kernels (ROCCO_FRAGFILE_THREADS), ROCCO_FRAGFILE_LINES_MAX_GRID,
 *   ROCCO_FRAGFILE_FIELDS_MAX_GRID, ROCCO_FRAGFILE_COUNT_MAX_GRID. */
#define ROCCO_FRAGFILE_THREADS 256
#define ROCCO_FRAGFILE_TILE_BYTES 4096
#define ROCCO_FRAGFILE_LINES_MAX_GRID 2048  /* unit: one tile of bytes (fragfile_line_facts_kernel, fragfile_line_emit_kernel) */
#define ROCCO_FRAGFILE_FIELDS_MAX_GRID 2048 /* unit: ROCCO_FRAGFILE_THREADS lines (fragfile_fields_kernel, fragfile_order_kernel) */
#define ROCCO_FRAGFILE_COUNT_MAX_GRID 1024  /* unit: ROCCO_FRAGFILE_THREADS lines (fragfile_count_kernel, fragfile_range_kernel, fragfile_mapped_kernel) */
#define ROCCO_FRAGFILE_SCAN_ITEMS 4         /* bins per thread of a scan tile (fragfile_finish_kernel: one workgroup per track) */
/* the status word of a line */
#define ROCCO_FRAGFILE_META 0x1u             /* begins with '#' */
#define ROCCO_FRAGFILE_FIELDS_SHIFT 1        /* bits 1..3: min(the fields the count rule's loop scans, 5) */
#define ROCCO_FRAGFILE_FIELDS_MASK 0x7u
#define ROCCO_FRAGFILE_START_OK 0x10u        /* column 2 parsed (and lies within int32) */
#define ROCCO_FRAGFILE_END_OK 0x20u          /* column 3 parsed */
#define ROCCO_FRAGFILE_LAST_EMPTY 0x40u      /* the count rule: the last field scanned is empty (2257) */
#define ROCCO_FRAGFILE_FIFTH_EMPTY 0x80u     /* the mapped rule: the fifth field is empty or absent (1812) */
#define ROCCO_FRAGFILE_WEIGHT_PARSED 0x100u  /* column 5 parsed */
#define ROCCO_FRAGFILE_BARCODE_PRESENT 0x200u
#define ROCCO_FRAGFILE_BARCODE_ALLOWED 0x400u /* the barcode is empty or absent, the list is empty, or it holds the barcode */
#define ROCCO_FRAGFILE_NONCANONICAL 0x800u   /* column 2 or 3 is no canonical decimal */
#define ROCCO_FRAGFILE_BEYOND 0x1000u        /* column 2, 3 or 5 at or beyond 2^31 (column 5: or more than 18 digits) */
/* what a line is refused for, lowest first */
#define ROCCO_FRAGFILE_ERR_FIELDS 1
#define ROCCO_FRAGFILE_ERR_NUL 2
#define ROCCO_FRAGFILE_ERR_CR 3
#define ROCCO_FRAGFILE_ERR_NONCANONICAL 4
#define ROCCO_FRAGFILE_ERR_BEYOND 5
#define ROCCO_FRAGFILE_ERR_COUNT 6
#define ROCCO_FRAGFILE_ERR_CONTIG 7
#define ROCCO_FRAGFILE_ERR_ORDER 8
/* the reference's ccounts_countMode */
#define ROCCO_FRAGFILE_MODE_COVERAGE 0
#define ROCCO_FRAGFILE_MODE_CUTSITE 1
#define ROCCO_FRAGFILE_MODE_FIVEPRIME 2
#define ROCCO_FRAGFILE_MODE_CENTER 3
typedef struct rocco_hip_fragfile_options {
    int32_t count_mode, one_read_per_bin;
} rocco_hip_fragfile_options;
int rocco_hip_fragfile_lines(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, size_t entry0, int64_t *starts_out_dev,
                             size_t capacity, int64_t *report_out_host, void *stream);
int rocco_hip_fragfile_fields(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines,
                              int whole_file, const int64_t *track_first_host, const int32_t *expect_host, size_t K,
                              const uint8_t *names_host, const int64_t *name_offsets_host, size_t n_names, const uint8_t *allow_bytes_dev,
                              const int64_t *allow_offsets_dev, size_t n_allow, const int64_t *allow_first_host, int32_t *start_out_dev,
                              int32_t *end_out_dev, int32_t *weight_out_dev, int32_t *name_out_dev, uint32_t *status_out_dev,
                              int64_t *report_out_host, void *stream);
int rocco_hip_fragfile_count_batch(rocco_hip_solver *solver, const int32_t *start_dev, const int32_t *end_dev, const int32_t *weight_dev,
                                   const uint32_t *status_dev, const int64_t *line_offsets_host, size_t K,
                                   const rocco_hip_fragfile_options *options_host, const rocco_hip_count_region *regions_host,
                                   const int64_t *out_offsets_host, float *out_dev, int64_t *max_magnitude_out_host, void *stream);
int rocco_hip_fragfile_chrom_range_batch(rocco_hip_solver *solver, const int32_t *start_dev, const int32_t *end_dev,
                                         const uint32_t *status_dev, const int64_t *line_offsets_host, const int64_t *chrom_len_host,
                                         size_t K, int64_t *range_out_host, void *stream);
int rocco_hip_fragfile_mapped_count(rocco_hip_solver *solver, const int32_t *weight_dev, const int32_t *name_dev, const uint32_t *status_dev,
                                    size_t n_lines, int count_mode, int one_read_per_bin, uint64_t *sum_out_host, void *stream);
int rocco_hip_fragfile_host(rocco_hip_solver *solver, const uint8_t *bytes, size_t n_bytes, size_t entry0, int64_t *starts_out, size_t capacity,
                            int64_t *lines_report_out, int whole_file, const int64_t *track_first, const int32_t *expect, size_t K,
                            const uint8_t *names, const int64_t *name_offsets, size_t n_names, const uint8_t *allow_bytes,
                            const int64_t *allow_offsets, size_t n_allow, const int64_t *allow_first, int32_t *start_out, int32_t *end_out,
                            int32_t *weight_out, int32_t *name_out, uint32_t *status_out, int64_t *fields_report_out);
void rocco_hip_fragfile_shape(int *shape_out);

/* ---- the barcode census of a fragments file (note (35)) -------------------------------------
 * ccounts_getCellCount (rocco/native/ccounts_backend.c:1890-2046): the distinct barcodes of a whole fragments file under an
 * optional allow-list -- here with the number of lines of every barcode besides.  The rule of a line (1937-1975; csrc/
 * fragments_rules.h, frag_barcode_field): fields end at '\t', the scan of the line ends at '\n', '\r' or NUL wherever they
 * stand, the barcode is field 3; a line whose scan ends before it, whose field 3 is empty (1964) or whose barcode the list
 * does not hold (1968-1975, ccounts_barcodeAllowed) contributes nothing.  A '#' line is a line; no other column is parsed,
 * so the dialect errors of rocco_hip_fragfile_fields do not apply.  The reference's khash set (1930, 1999) is replaced by:
 *
 * the table: `capacity` (a power of two >= ROCCO_BARCODE_CENSUS_MIN_CAPACITY) 64-bit slots and as many 64-bit counters,
 *   caller-owned and zeroed before their first use; a slot is 0 (empty) or bit 63 | a 24-bit tag of the masked hash << 39 |
 *   bit 38 (the payload is an arena entry; clear: a line of the slab in flight) | the index.  The arena: the bytes of the
 *   barcodes settled so far one behind the other, their entries + 1 offsets (arena_offsets_dev[0] = 0) and their full
 *   64-bit hashes (frag_hash64).  It persists across the slabs of a file.
 * rocco_hip_barcode_census_insert: one slab.  One lane per line of starts_dev[n_lines + 1] (ROCCO_FRAGFILE_THREADS lines per
 *   workgroup turn, a grid stride under ROCCO_BARCODE_CENSUS_MAX_GRID) hashes its barcode, ANDs the hash with hash_mask and
 *   probes linearly from there: one compare-and-swap on an empty slot; a lane that loses it or finds the slot taken compares
 *   bytes through the word the atomic returned (the slab's text and the arena were written before the launch) and adds 1 to
 *   the slot's counter on equal bytes, probes the next slot otherwise.  No lane waits for another; slot words are read
 *   through agent-scope atomics only.  Then hipcub's exclusive sum over the winners' lengths and a settle kernel copy the new
 *   representatives into the arena and rewrite their slots to arena form, so that the slab may be released when the call
 *   returns.  Required (ROCCO_HIP_EINVAL otherwise): capacity >= 2 * (entries + n_lines), arena_entries_capacity >= entries +
 *   n_lines, arena_bytes_capacity >= arena_used + n_bytes, n_lines < 2^26, n_bytes < 2^38.  With that bound every probe ends;
 *   a probe of `capacity` steps raises a flag and the call fails with ROCCO_HIP_EINVAL.  allow_*: one sorted packed list, n_allow == 0 for none.
 *   report_out_host[0..3] = new entries, the bytes they added to the arena, 0, 0.
 * rocco_hip_barcode_census_rehash: the entries of a table into a larger zeroed-by-this-call table by their stored hashes
 *   (no barcode byte is read), counters with them.
 * rocco_hip_barcode_census_records: records_out_dev[e] = the counter of entry e, for the `entries` entries.
 * rocco_hip_barcode_census_host: the same census over HOST memory on the calling thread, all lines of `bytes` at once, from
 *   the same header (test support; `solver` may be NULL): a sequential table of initial_capacity slots (raised to the
 *   minimum) that grows under the same bound.  Entries in the order of their first line.  With the three outputs NULL only
 *   the report is made: report_out[0..3] = entries, the bytes of all barcodes, lines, grows.
 * rocco_hip_barcode_census_shape: shape_out[0..3] = ROCCO_FRAGFILE_THREADS, the lines of a workgroup turn (the same),
 *   ROCCO_BARCODE_CENSUS_MAX_GRID, ROCCO_BARCODE_CENSUS_MIN_CAPACITY. */
#define ROCCO_BARCODE_CENSUS_MAX_GRID 1024   /* unit: ROCCO_FRAGFILE_THREADS lines or slots (every kernel of barcode_census.hip) */
#define ROCCO_BARCODE_CENSUS_MIN_CAPACITY 64 /* slots */
int rocco_hip_barcode_census_insert(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines,
                                    const uint8_t *allow_bytes_dev, const int64_t *allow_offsets_dev, size_t n_allow, uint64_t *slots_dev,
                                    int64_t *counts_dev, size_t capacity, uint8_t *arena_bytes_dev, size_t arena_bytes_capacity,
                                    int64_t *arena_offsets_dev, uint64_t *arena_hashes_dev, size_t arena_entries_capacity, size_t entries,
                                    size_t arena_used, uint64_t hash_mask, int64_t *report_out_host, void *stream);
int rocco_hip_barcode_census_rehash(rocco_hip_solver *solver, const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity,
                                    uint64_t *new_slots_dev, int64_t *new_counts_dev, size_t new_capacity, const uint64_t *arena_hashes_dev,
                                    size_t entries, uint64_t hash_mask, void *stream);
int rocco_hip_barcode_census_records(rocco_hip_solver *solver, const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity,
                                     size_t entries, int64_t *records_out_dev, void *stream);
int rocco_hip_barcode_census_host(rocco_hip_solver *solver, const uint8_t *bytes, size_t n_bytes, const uint8_t *allow_bytes,
                                  const int64_t *allow_offsets, size_t n_allow, uint64_t hash_mask, size_t initial_capacity, uint8_t *bytes_out,
                                  size_t bytes_capacity, int64_t *offsets_out, int64_t *records_out, size_t entries_capacity,
                                  int64_t *report_out);
void rocco_hip_barcode_census_shape(int *shape_out);

/* ---- the grid caps of the record and select kernels -----------------------------------------------------------------
 * Every kernel behind the data front end caps its grid; past cap x unit a workgroup takes several units in turn (a grid
 * stride).  The caps are stated here once, the .hip files are built to them, and rocco_hip_launch_caps hands them to the
 * tests, which size themselves from them to reach a second turn (tests/test_gpu_launch_turns.py).  A "unit" is what one
 * workgroup takes per turn.
 *
 * The select (select.hip) has no fixed cap: a counting pass has about ROCCO_SELECT_GRID_TARGET workgroups for a group of
 * up to 48 vectors, dealt to the vectors by length.  Vector v of n_v values has chunks = ceil(n_v / ROCCO_SELECT_CHUNK_VALUES)
 * and gets
 *     blocks = min(chunks, floor(ROCCO_SELECT_GRID_TARGET * n_v / group_total) + 1)      (the product and quotient in double)
 * workgroups, group_total = the sum of the group's n_v; workgroup j of the vector counts its chunks j, j + blocks, ... into
 * ONE LDS histogram.  A vector is in its second turn when blocks < chunks. */
#define ROCCO_SELECT_GRID_TARGET 1024      /* unit: one chunk of ROCCO_SELECT_CHUNK_VALUES values of one vector (select_count_kernel) */
#define ROCCO_SELECT_CHUNK_VALUES 16384    /* values of a chunk */
#define ROCCO_SELECT_THREADS 256           /* threads of a counting workgroup */
#define ROCCO_BH_MAX_GRID 2048             /* unit: ROCCO_BH_THREADS sorted p-values (bh_last_passing_kernel) */
#define ROCCO_BH_THREADS 256
#define ROCCO_COUNT_THREADS 256            /* threads per workgroup of count.hip's kernels */
#define ROCCO_CHROM_RANGE_MAX_GRID 2048    /* unit: ROCCO_COUNT_THREADS records (chrom_range_kernel) */
#define ROCCO_COUNT_TAIL_MAX_GRID 4096     /* unit: ROCCO_COUNT_THREADS bins (count_tail_kernel) */
#define ROCCO_COUNT_INTERVALS_THREADS 256  /* threads per workgroup of interval_count.hip's kernels */
#define ROCCO_INTERVAL_FACTS_MAX_GRID 2048 /* unit: ROCCO_COUNT_INTERVALS_THREADS records (interval_track_facts_kernel) */
#define ROCCO_FRAGMENT_MAX_GRID 2048       /* unit: ROCCO_FRAGMENT_THREADS records (record_flag_facts_kernel, template_length_kernel); ROCCO_FRAGMENT_DENSITY_RECORDS records (chunk_density_kernel) */
#define ROCCO_BAM_MAX_GRID 4096            /* unit: one segment (bam_guess_kernel); ROCCO_BAM_THREADS segments (bam_walk_kernel, bam_emit_kernel); ROCCO_BAM_THREADS records (bam_fields_kernel, bam_stream_firsts_kernel) */
/* rocco_hip_launch_caps: out[0 .. ROCCO_LAUNCH_CAPS) = ROCCO_SELECT_GRID_TARGET, ROCCO_SELECT_CHUNK_VALUES, ROCCO_SELECT_THREADS,
 * ROCCO_BH_MAX_GRID, ROCCO_BH_THREADS, ROCCO_CHROM_RANGE_MAX_GRID, ROCCO_COUNT_TAIL_MAX_GRID, ROCCO_COUNT_THREADS,
 * ROCCO_INTERVAL_FACTS_MAX_GRID, ROCCO_COUNT_INTERVALS_THREADS, ROCCO_FRAGMENT_MAX_GRID, ROCCO_FRAGMENT_THREADS,
 * ROCCO_FRAGMENT_DENSITY_RECORDS, ROCCO_FRAGMENT_DENSITY_WINDOW, ROCCO_BAM_MAX_GRID, ROCCO_BAM_THREADS. */
#define ROCCO_LAUNCH_CAPS 16
void rocco_hip_launch_caps(int *out);

/* ---- synthetic signal matrices (benchmark / test support, device-resident) -------------------
 * Fills a row-major [K][n] matrix with the counter-based synthetic tracks described in
 * DESIGN.md section 7 (5-decimal background + planted peaks with per-sample dropout); the same
 * integer arithmetic is restated in NumPy in rocco_amd/synth.py so any slice can be regenerated
 * on the host bit-for-bit. */
int rocco_hip_synth_matrix(rocco_hip_solver *solver, void *matrix_dev, int dtype, size_t K, size_t n,
                           size_t row_stride, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROCCO_HIP_H */
